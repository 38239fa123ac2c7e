"""Route cases of gemm_rowpanel.hip / ff_fused.hip on the GPU: which instantiation ran, and is every output element right.

The sibling of tools/route_check.py (whose guarded buffers, profiler capture, bound and statistics checks it uses) for ROWPANEL_CASES of
tests/route_cases.py.  One process per environment (tests/test_kernel_routes.py starts both):
    --env hook      AE_ROWPANEL_ANY_M=1 and no other AE_* variable: the small cases, one 192-row block is enough;
    --env default   no AE_* variable: the plan threshold from both sides (192 blocks run the kernels, 191 full blocks run gemm_kernel).
For each case:
  1. seeded bf16 operands (tests/rowpanel_ref.py); the ops run once under torch.profiler -> the kernel names, which must include every
     instantiation whose ROWPANEL_LEDGER row lists the case (a `tiled` case: a gemm_kernel and neither of the two files' kernels);
  2. every output and statistics buffer is a view inside a sentinel-filled allocation (rows before and after, columns beside an output
     that is a slice of a wider buffer): the guards must be unchanged and no sentinel may be left inside;
  3. a second run into fresh buffers must be bit-identical;
  4. ALL elements are checked against float64 on the same bf16 operands; the bounds and their derivation are in tests/rowpanel_ref.py.
     A producer's output with row statistics must equal the launch without them bit for bit; a LayerNorm fold is referred to the rows and
     statistics its producer stored, the projection behind the feed-forward to the feed-forward output the same operands store without
     it.  The feed-forward is referred twice: to the hidden activation ops.ln_gemm stores (`output`, the bound widened by what two correct
     kernels may store differently) and to its own, which a launch with a 0/1 selection for W2 stores exactly (`hidden_own` against
     float64, `output_own` with the tight bound; `differing_hidden` counts where the two hidden activations differ, reported).
     ops.pack_ln_fold's (W', s, c) are checked against their definition.
After the first HIP / runtime error no further case starts; the summary then carries `aborted` and the exit status is non-zero.

    python tools/rowpanel_route_check.py --env hook|default [case-id-substring ...]     # one line per case, then `ROWPANEL_ROUTE_SUMMARY {json}`
"""
import json
import os
import re
import sys
import time
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import route_cases as RC  # noqa: E402
import rowpanel_ref as RR  # noqa: E402
from route_check import BF, CaseFailure, Guarded, _stats_with_tail, profiled, route_keys, stats_check  # noqa: E402

F32, F64 = torch.float32, torch.float64
K = RR.K
EPS = 1e-5
FAMILIES = re.compile(r"\b(gemm_rowpanel_kernel|ff_fused_kernel|gemm_kernel)<([^<>]*)>")


def _out(M, n, cpad=0):
    """guarded bf16 [M, n]; cpad: a column slice (8 columns in) of a buffer cpad + 8 columns wider"""
    return Guarded(M, n, BF, ld=n + cpad + 8, col0=8) if cpad else Guarded(M, n, BF)


def _wide(t, ld, col0=0):
    """`t` [M, n] on the GPU as columns col0 .. col0 + n of a seeded [M, ld] buffer"""
    buf = torch.randn(t.shape[0], ld, generator=torch.Generator().manual_seed(ld)).to(BF).cuda()
    buf[:, col0:col0 + t.shape[1]] = t.cuda()
    return buf[:, col0:col0 + t.shape[1]]


def _dev(t):
    return None if t is None else t.cuda()


def _colstats_check(st, y, what="column statistics"):
    return stats_check(st.view.cpu(), y, 32, what)


# --------------------------------------------------------------------------------------------------- plain / LayerNorm prologue
def build_rp(c, ops, gen):
    M, N, geglu, lnm = c["M"], c["N"], c["epi"] == "geglu", c["lnm"]
    n_out = N // 2 if geglu else N
    epi = ops.EPI_GEGLU if geglu else ops.EPI_NONE
    x = RR.make_rows(gen, M)
    w = RR.make_weight(gen, N, K).to(BF)
    b = RR.make_bias(gen, N) if c.get("bias", True) else None
    gamma, beta = RR.make_affine(gen) if lnm else (None, None)
    res = torch.randn(M, n_out, generator=gen).to(BF) if c.get("res") else None
    a_d = _wide(x, 3 * K, K) if c.get("aslice") else x.cuda()
    if geglu:       # reference: chunk(2) of the unpacked projection; the kernel takes ops.pack_geglu's layout
        w_d, b_d = ops.pack_geglu(w.cuda(), (b if b is not None else torch.zeros(N)).cuda())
        b_d = b_d if b is not None else None
    else:
        w_d, b_d = w.cuda(), _dev(b)
    r_d = None if res is None else (_wide(res, n_out + c["ldr"]) if c.get("ldr") else res.cuda())
    g_d, be_d = _dev(gamma), _dev(beta)

    def launch():
        o = _out(M, n_out, c.get("cpad", 0))
        st = _stats_with_tail((M + 31) // 32, n_out) if c.get("cs") else None
        kw = dict(residual=r_d, epilogue=epi, out=o.view, colstats=st.view if st else None)
        if lnm:
            ops.ln_gemm(a_d, g_d, be_d, EPS, w_d, b_d, **kw)
        else:
            ops.gemm(a_d, w_d, bias=b_d, **kw)
        return dict(y=o, colstats=st)

    def check(outs):
        y = outs["y"].view.cpu()
        if lnm:
            ref, bnd, share = RR.ln_gemm_ref(x, gamma, beta, EPS, w, b, res, geglu)
            if share > RR.AMBIGUOUS_CAP:
                raise CaseFailure(f"{share:.3f} of the LayerNorm operands are ambiguous")
        else:
            ref, bnd = RR.gemm_ref(x, w, b, res, geglu)
        r = dict(output=RR.check(y, ref, bnd, "output"))
        if outs["colstats"] is not None:
            r["colstats"] = _colstats_check(outs["colstats"], y)
        return r

    return dict(launch=launch, check=check)


# --------------------------------------------------------------------------------------------------- producer with row statistics, LayerNorm fold
def _producer(c, ops, gen, N):
    M = c["M"]
    a = torch.randn(M, K, generator=gen).to(BF)
    w = RR.make_weight(gen, N, K).to(BF)
    b = RR.make_bias(gen, N)
    r = RR.make_rows(gen, M, N) if c.get("res", True) else None
    a_d, w_d, b_d, r_d = a.cuda(), w.cuda(), b.cuda(), _dev(r)

    def launch():
        o, plain = Guarded(M, N, BF), Guarded(M, N, BF)
        rs = Guarded(M, N // 64, F32, trailing=(2,))
        ops.gemm(a_d, w_d, bias=b_d, residual=r_d, out=o.view, rowstats=rs.view)
        ops.gemm(a_d, w_d, bias=b_d, residual=r_d, out=plain.view)
        return dict(x=o, x_plain=plain, rowstats=rs)

    def check(outs):
        x = outs["x"].view.cpu()
        if not torch.equal(outs["x"].bits(), outs["x_plain"].bits()):
            raise CaseFailure("the row-statistics epilogue changed the GEMM's output")
        ref, bnd = RR.gemm_ref(a, w, b, r)
        return dict(output=RR.check(x, ref, bnd, "producer output"), rowstats=RR.row_stats_check(outs["rowstats"].view.cpu(), x))

    return launch, check


def build_rs(c, ops, gen):
    launch, check = _producer(c, ops, gen, c["N"])
    return dict(launch=launch, check=check)


def build_chain(c, ops, gen):
    M, N, geglu = c["M"], c["N"], c["epi"] == "geglu"
    n_out = N // 2 if geglu else N
    p_launch, p_check = _producer(dict(M=M, res=True), ops, gen, K)
    w = RR.make_weight(gen, N, K)
    b = RR.make_bias(gen, N)
    gamma, beta = RR.make_affine(gen)
    res = torch.randn(M, n_out, generator=gen).to(BF) if c.get("res") else None
    wq, s, cc = ops.pack_ln_fold(w.cuda(), b.cuda(), gamma.cuda(), beta.cuda(), geglu=geglu)
    r_d = _dev(res)
    epi = ops.EPI_GEGLU if geglu else ops.EPI_NONE

    def launch():
        outs = p_launch()
        o = Guarded(M, n_out, BF)
        ops.gemm_ln(outs["x"].view, outs["rowstats"].view, wq, s, cc, EPS, residual=r_d, epilogue=epi, out=o.view)
        outs["y"] = o
        return outs

    def check(outs):
        r = p_check(outs)
        r = dict(producer=r["output"], rowstats=r["rowstats"])
        # the packed operands against their definition (W' one bf16 rounding of W gamma; s, c fp32 sums)
        wr, sr, cr = RR.pack_ln_fold_ref(w, b, gamma, beta, geglu, ops.pack_geglu)
        wd, sd, cd = wq.cpu(), s.cpu(), cc.cpu()
        if not torch.equal(wd.view(torch.int16), wr.view(torch.int16)):
            raise CaseFailure("pack_ln_fold: W' is not bf16(W gamma) in the packed row order")
        wa = wr.to(F64).abs().sum(1)
        ca = RR.pack_ln_fold_ref(w.abs(), b.abs(), gamma, beta.abs(), geglu, ops.pack_geglu)[2].to(F64)
        r["pack"] = max(RR.check(sd[None], wr.to(F64).sum(1)[None], RR.A_ACC * wa[None] + 1e-30, "pack_ln_fold s"),
                        RR.check(cd[None], cr.to(F64)[None], 2.0 ** -20 * cr.to(F64).abs()[None] + RR.A_ACC * ca[None] + 1e-30, "pack_ln_fold c"))
        ref, bnd = RR.fold_ref(outs["x"].view.cpu(), wd, sd, cd, EPS, res, geglu)
        r["output"] = RR.check(outs["y"].view.cpu(), ref, bnd, "folded output")
        return r

    return dict(launch=launch, check=check)


# --------------------------------------------------------------------------------------------------- fused feed-forward
def build_ff(c, ops, gen):
    M, H, C, proj, strided, tiled = c["M"], c["H"], K, c["proj"], c["strided"], c.get("tiled", False)
    x = RR.make_rows(gen, M)
    w1 = RR.make_weight(gen, 2 * H, C).to(BF)
    b1 = RR.make_bias(gen, 2 * H)
    w2 = RR.make_weight(gen, C, H)
    b2 = RR.make_bias(gen, C)
    gamma, beta = RR.make_affine(gen)
    res = torch.randn(M, C, generator=gen).to(BF) if c["res"] else None
    w3 = b3 = r3 = None
    if proj:
        w3 = RR.make_weight(gen, C, C).to(BF)
        b3 = RR.make_bias(gen, C) if proj["b3"] else None
        r3 = torch.randn(M, C, generator=gen).to(BF) if proj["r3"] else None
    w1p, b1p = ops.pack_geglu(w1.cuda(), b1.cuda())
    w2img = ops.pack_ff2_fused(w2.cuda())
    x_d = _wide(x, 3 * C, C) if strided else x.cuda()
    r_d = None if res is None else (_wide(res, C + 328) if strided else res.cuda())
    r3_d = None if r3 is None else (_wide(r3, C + 32) if strided else r3.cuda())
    if strided:
        w1p = _wide(w1p, C + 8)
    g_d, be_d, b2_d, w3_d, b3_d = gamma.cuda(), beta.cuda(), b2.cuda(), _dev(w3), _dev(b3)
    w2_d = w2.to(BF).cuda()
    fused = bool(ops.ff_fused_ok(M, C, H))
    # W2 := a 0/1 selection of hidden units 320 p .. 320 p + 319, b2 = 0, no residual: the fused kernel then stores its own hidden activation exactly
    sel = []
    for p in range((H + C - 1) // C):
        n = min(C, H - C * p)
        s2 = torch.zeros(C, H)
        s2[torch.arange(n), C * p + torch.arange(n)] = 1.0
        sel.append((n, ops.pack_ff2_fused(s2.cuda())))

    def launch():
        if fused == tiled:
            raise CaseFailure(f"ff_fused_ok({M}, {C}, {H}) is {fused}: the case expects the " + ("tiled kernels" if tiled else "fused kernel"))
        y, h = _out(M, C, 16 if strided else 0), Guarded(M, H, BF)
        ops.ln_gemm(x_d, g_d, be_d, EPS, w1p, b1p, epilogue=ops.EPI_GEGLU, out=h.view)
        if fused:
            ops.ff_fused(x_d, g_d, be_d, EPS, w1p, b1p, w2img, b2_d, residual=r_d, out=y.view)
        else:       # what the block runs below the plan threshold: the GEGLU projection, then ff2 on the stored hidden activation
            ops.gemm(h.view, w2_d, bias=b2_d, residual=r_d, out=y.view)
        outs = dict(y=y, h=h, z=None, colstats=None)
        if fused:
            for p, (n, img) in enumerate(sel):
                outs[f"own{p}"] = Guarded(M, C, BF)
                ops.ff_fused(x_d, g_d, be_d, EPS, w1p, b1p, img, None, out=outs[f"own{p}"].view)
        if proj:
            outs["z"] = _out(M, C, 16 if strided else 0)
            outs["colstats"] = _stats_with_tail((M + 31) // 32, C) if proj["cs"] else None
            ops.ff_fused(x_d, g_d, be_d, EPS, w1p, b1p, w2img, b2_d, residual=r_d, out=outs["z"].view, w3=w3_d, b3=b3_d, residual3=r3_d,
                         colstats=outs["colstats"].view if proj["cs"] else None)
        return outs

    def check(outs):
        h_s, y_s = outs["h"].view.cpu(), outs["y"].view.cpu()
        ref, bnd, share = RR.ln_gemm_ref(x, gamma, beta, EPS, w1, b1, None, True)
        if share > RR.AMBIGUOUS_CAP:
            raise CaseFailure(f"{share:.3f} of the LayerNorm operands are ambiguous")
        r = dict(hidden=RR.check(h_s, ref, bnd, "stored hidden activation"))
        if fused:      # the kernel's own hidden activation: against float64, and the output against it with the tight bound
            own = [outs[f"own{p}"].view.cpu() for p in range(len(sel))]
            if any(n < C and bool(o[:, n:].float().abs().any()) for (n, _), o in zip(sel, own)):
                raise CaseFailure("a 0/1 selection W2 left something in the columns it does not select")
            h_f = torch.cat([o[:, :n] for (n, _), o in zip(sel, own)], 1)
            r["hidden_own"] = RR.check(h_f, ref, bnd, "the fused kernel's own hidden activation")
            r["_differing_hidden"] = int((h_f.view(torch.int16) != h_s.view(torch.int16)).sum())
            ref_o, bnd_o = RR.gemm_ref(h_f, w2.to(BF), b2, res)
            r["output_own"] = RR.check(y_s, ref_o, bnd_o, "feed-forward output (own hidden activation)")
            dev = RR.hidden_deviation(ref, bnd)
        else:          # ff2 reads h_s itself
            dev = None
        ref, bnd = RR.gemm_ref(h_s, w2.to(BF), b2, res, dev=dev)
        r["output"] = RR.check(y_s, ref, bnd, "feed-forward output")
        if proj:
            z = outs["z"].view.cpu()
            ref, bnd = RR.gemm_ref(y_s, w3, b3, r3)
            r["proj"] = RR.check(z, ref, bnd, "projection output")
            if outs["colstats"] is not None:
                r["colstats"] = _colstats_check(outs["colstats"], z)
        return r

    return dict(launch=launch, check=check)


BUILD = dict(rp=build_rp, rs=build_rs, chain=build_chain, ff=build_ff)
OURS = ("gemm_rowpanel_kernel<", "ff_fused_kernel<")


# --------------------------------------------------------------------------------------------------- driver
def run_case(c, ops):
    gen = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    spec = BUILD[c["op"]](c, ops, gen)
    res = dict(id=c["id"], kernels=[], keys=[], ok=False, ratio=None, parts=None, guards=None, error=None)
    try:
        outs1, names = profiled(spec["launch"])
        names, keys = route_keys(names, FAMILIES)
        res["kernels"], res["keys"] = names, sorted(set(keys))
        missing = [k for k in RC.expected_kernels(c["id"]) if k not in keys]
        if missing:
            raise CaseFailure(f"declared instantiation(s) not reached: {missing}")
        if c.get("tiled") and (any(k.startswith(OURS) for k in keys) or not any(k.startswith("gemm_kernel<") for k in keys)):
            raise CaseFailure(f"below the plan threshold the tiled gemm_kernel must run, got {sorted(set(keys))}")
        outs2 = spec["launch"]()
        torch.cuda.synchronize()
        gd = all(g.guards_intact() for o in (outs1, outs2) for g in o.values() if g is not None)
        res["guards"] = "intact" if gd else "CLOBBERED"
        if not gd:
            raise CaseFailure("a guard area was written")
        for name, g in outs1.items():
            if g is None:
                continue
            if not torch.equal(g.bits(), outs2[name].bits()):
                raise CaseFailure(f"{name}: two runs differ")
            left = int((g.bits() == g.sent).sum())
            if left:
                raise CaseFailure(f"{name}: {left} elements were never written")
        parts = spec["check"](outs1)
        res["info"] = {k[1:]: v for k, v in parts.items() if k.startswith("_")}      # counts that are reported, not bounded
        res["parts"] = {k: v for k, v in parts.items() if not k.startswith("_")}
        res["ratio"], res["ok"] = max(res["parts"].values()), True
    except CaseFailure as e:
        res["error"] = str(e)
    return res


def main():
    args = sys.argv[1:]
    if len(args) < 2 or args[0] != "--env" or args[1] not in ("hook", "default"):
        print(__doc__.strip().splitlines()[-1], flush=True)
        sys.exit(2)
    env, flt = args[1], args[2:]
    want = {"AE_ROWPANEL_ANY_M": "1"} if env == "hook" else {}
    have = {k: v for k, v in os.environ.items() if k.startswith("AE_") and k != "AE_LIB_PATH"}
    if have != want:
        print(f"rowpanel_route_check: --env {env} runs with the AE_* variables {want}, got {have}", flush=True)
        sys.exit(2)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from anyedit_amd import ops
    cases = [c for c in RC.ROWPANEL_CASES if c["env"] == env and (not flt or any(f in c["id"] for f in flt))]
    results, t0 = [], time.time()
    aborted = None
    for c in cases:
        t1 = time.time()
        try:
            r = run_case(c, ops)
        except Exception as e:   # a HIP / runtime error: start no further GPU work
            aborted = dict(id=c["id"], error=f"{type(e).__name__}: {e}")
            print(f"ABORT {c['id']}: {aborted['error']}", flush=True)
            break
        results.append(r)
        parts = " ".join([f"{k} {v:.3f}" for k, v in (r["parts"] or {}).items()] + [f"{k} {v}" for k, v in (r.get("info") or {}).items()])
        print(f"{'PASS' if r['ok'] else 'FAIL'} {r['id']:28s} {time.time() - t1:5.1f}s worst {r['ratio'] if r['ratio'] is None else round(r['ratio'], 3)} [{parts}] "
              f"guards {r['guards']} kernels {r['keys'] or r['kernels']}" + (f"  ERROR {r['error']}" if r["error"] else ""), flush=True)
    byid = {r["id"]: r for r in results}
    per_kernel = {}
    for key, (_, ids) in RC.ROWPANEL_LEDGER.items():
        rt = [byid[i]["ratio"] for i in ids if i in byid and byid[i]["ratio"] is not None]
        if rt:
            per_kernel[key] = max(rt)
            print(f"worst error / bound  {key:42s} {max(rt):.3f}  ({len(rt)} cases)", flush=True)
    summary = dict(env=env, results=results, aborted=aborted, per_kernel=per_kernel, seconds=round(time.time() - t0, 1))
    print("ROWPANEL_ROUTE_SUMMARY " + json.dumps(summary), flush=True)
    sys.exit(0 if aborted is None and all(r["ok"] for r in results) else 1)


if __name__ == "__main__":
    main()
