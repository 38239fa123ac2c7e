"""Route cases of norm.hip on the GPU: which GroupNorm / LayerNorm kernel ran, and is every output element right.

The sibling of tools/route_check.py (whose guarded buffers and profiler capture it uses) for NORM_CASES of tests/route_cases.py; one process,
no AE_* routing variable set (tests/test_kernel_routes.py starts it that way).  For each case:
  1. seeded bf16 operands with statistics of their own per (sample, group) (tests/norm_ref.py); the op runs through `ops` once under
     torch.profiler -> the kernel names of that case, which must include every instantiation whose NORM_LEDGER row lists the case;
  2. every output — y, stat_out, xsum, dx / dx2, dgamma / dbeta — is a view inside a sentinel-filled allocation: the guard areas must be
     unchanged and no sentinel may be left inside (accumulate targets are pre-filled with a seeded gradient instead);
  3. a second run on fresh buffers must be bit-identical;
  4. (mean, rstd) are checked on their own where the route delivers them (GroupNorm's stat_out);
  5. ALL elements of every output are checked against float64 on the same bf16 operands.
The bounds of 4 and 5 and their derivation are in the docstring of tests/norm_ref.py; which statistics allowance applies (two-pass: the slab
kernels and every LayerNorm; one-pass: three launches and producer statistics) follows from the kernels that ran.  The padding rows of the
window partition must be exactly zero; the residual sum of the un-partition (xsum = bf16(windows + shortcut)) is an output of its own,
within one bf16 rounding of the float64 sum, and the LayerNorm behind it is referred to the sum as stored.

After the cases, the conditioning sweep (reported, nothing asserted): one GroupNorm shape per route family at |mean| / sigma in
{8, 16, 32, 64, 128, 256} and the worst |rstd^ / rstd - 1| of each, printed as `CONDITIONING {json}` (DESIGN.md holds the table).

    python tools/norm_route_check.py [case-id-substring ...]      # one line per case, then `NORM_ROUTE_SUMMARY {json}`
"""
import json
import os
import re
import subprocess
import sys
import time
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import norm_ref as NR  # noqa: E402
import route_cases as RC  # noqa: E402
from route_check import BF, CaseFailure, Guarded, profiled  # noqa: E402

F32 = torch.float32
FAMILIES = re.compile(r"\b(gn_slab_kernel|gn_apply_kernel|gnb_slab_kernel|layernorm_rows_kernel|layernorm_kernel|layernorm_window_kernel|"
                      r"layernorm_narrow_kernel|layernorm_bwd_kernel)<([^<>]*)>")
PLAIN = re.compile(r"\b(gn_stats_kernel|gn_finalize_kernel|gn_finalize_cs_kernel|gnb_partial_kernel|gnb_finalize_kernel|gnb_apply_kernel|"
                   r"layernorm_param_grad_kernel)\b")
SWEEP = (8.0, 16.0, 32.0, 64.0, 128.0, 256.0)


def norm_keys(names):
    mangled = [n for n in names if n.startswith("_Z")]
    if mangled:
        dm = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True).stdout.split("\n")
        table = dict(zip(mangled, dm))
        names = [table.get(n, n) for n in names]
    keys = []
    for n in names:
        m = FAMILIES.search(n)
        if m:
            keys.append(f"{m.group(1)}<{', '.join(x.strip() for x in m.group(2).split(','))}>")
        else:
            m = PLAIN.search(n)
            if m:
                keys.append(m.group(1))
    return names, keys


def vec(n):
    """guarded fp32 [n]"""
    g = Guarded(1, n, F32, guard=64)
    g.vec = g.view[0]
    return g


def filled(rows, cols, old):
    """guarded bf16 [rows, cols] that already holds the gradient `old` (an accumulate target)"""
    g = Guarded(rows, cols, BF)
    g.view.copy_(old)
    return g


# --------------------------------------------------------------------------------------------------- GroupNorm
def _gn_operands(c, gen, ratio=None):
    B, HW, C, G, C1 = c["B"], c["HW"], c["C"], c["groups"], c["C1"]
    x = NR.make_x(gen, B, HW, C, G, ratio=ratio, const_group=ratio is None)
    gamma, beta = NR.make_affine(gen, C)
    x2d = x.reshape(B * HW, C)
    xa = (x2d[:, :C1].contiguous() if C1 else x2d).cuda()
    xb = x2d[:, C1:].contiguous().cuda() if C1 else None
    return x, gamma, beta, x2d, xa, xb


def build_gn(c, ops, gen, ratio=None):
    B, HW, C, G, C1 = c["B"], c["HW"], c["C"], c["groups"], c["C1"]
    eps, act = 1e-5, 1 if c["silu"] else 0
    x, gamma, beta, x2d, xa, xb = _gn_operands(c, gen, ratio)
    gd, bd = gamma.cuda(), beta.cuda()
    csa = csb = None
    if c["cs"]:
        csa = NR.slab_sums(x2d[:, :C1] if C1 else x2d).cuda()
        csb = NR.slab_sums(x2d[:, C1:]).cuda() if C1 else None

    def launch():
        o = Guarded(B * HW, C, BF)
        st = Guarded(B, G, F32, trailing=(2,)) if c["stat"] else None
        ops.groupnorm(xa, gd, bd, B, HW, eps, silu=c["silu"], groups=G, x2=xb, out=o.view, stat_out=st.view if st else None,
                      colstats=csa, colstats2=csb)
        return dict(y=o, stat=st)

    def check(outs, keys):
        onepass = not any(k.startswith("gn_slab_kernel") for k in keys)
        f = NR.forward(x, gamma, beta, G, eps, act, onepass)
        r = {}
        if outs["stat"] is not None:
            r["stat"] = NR.check_statistics(outs["stat"].view.cpu(), f["mean"], f["rstd"], onepass)
        r["out"] = NR.check_elements(outs["y"].view.cpu().reshape(B, HW, C), f["y"], f["bnd"], "output")
        return r

    return dict(launch=launch, check=check, acc=(), x=x, eps=eps)


def build_gnb(c, ops, gen):
    B, HW, C, G, C1 = c["B"], c["HW"], c["C"], c["groups"], c["C1"]
    eps, act, acc = 1e-5, 1 if c["silu"] else 0, c["acc"]
    x, gamma, beta, x2d, xa, xb = _gn_operands(c, gen)
    gd, bd = gamma.cuda(), beta.cuda()
    dy = torch.randn(B * HW, C, generator=gen).to(BF)
    old = torch.randn(B * HW, C, generator=gen).to(BF)
    Ca = C1 or C
    mask = torch.zeros(C)
    if acc & 1:
        mask[:Ca] = 1.0
    if acc & 2:
        mask[Ca:] = 1.0
    old = (old.float() * mask).to(BF)
    dyd, oldd = dy.cuda(), old.cuda()

    def launch():
        st = None
        if c["saved"]:
            st = Guarded(B, G, F32, trailing=(2,))
            ops.groupnorm(xa, gd, bd, B, HW, eps, silu=c["silu"], groups=G, x2=xb, stat_out=st.view)
        d1 = filled(B * HW, Ca, oldd[:, :Ca]) if acc & 1 else Guarded(B * HW, Ca, BF)
        d2 = (filled(B * HW, C - Ca, oldd[:, Ca:]) if acc & 2 else Guarded(B * HW, C - Ca, BF)) if C1 else None
        kw = dict(dx_into=d1.view) if acc & 1 else dict(dx_out=d1.view)
        if C1:
            kw.update(dict(dx2_into=d2.view) if acc & 2 else dict(dx2_out=d2.view))
        ops.groupnorm_bwd(xa, gd, bd, dyd, B, HW, eps, silu=c["silu"], groups=G, x2=xb, stat=st.view if st else None, **kw)
        return dict(dx=d1, dx2=d2, stat=st)

    def check(outs, keys):
        onepass = not any(k.startswith("gn_slab_kernel") for k in keys)     # the route of the forward that saved the statistics; its own pass: one-pass
        b = NR.backward(x, gamma, beta, dy.reshape(B, HW, C), G, eps, act, onepass, old=old.reshape(B, HW, C) if acc else None, acc_mask=mask)
        r = {}
        if outs["stat"] is not None:
            m, rs = NR.statistics(x, G, eps)
            r["stat"] = NR.check_statistics(outs["stat"].view.cpu(), m, rs, onepass)
        got = outs["dx"].view.cpu() if not C1 else torch.cat([outs["dx"].view.cpu(), outs["dx2"].view.cpu()], 1)
        r["out"] = NR.check_elements(got.reshape(B, HW, C), b["dx"], b["bnd"], "dx" if not C1 else "[dx | dx2]")
        return r

    return dict(launch=launch, check=check, acc=tuple(n for n, bit in (("dx", 1), ("dx2", 2)) if acc & bit))


# --------------------------------------------------------------------------------------------------- LayerNorm
def _params(gamma, beta, aligned=True):
    if aligned:
        return gamma.cuda(), beta.cuda()
    out = []
    for t in (gamma, beta):     # 4 bytes past a 16-byte boundary
        buf = torch.empty(t.numel() + 1, dtype=F32, device="cuda")
        buf[1:].copy_(t)
        out.append(buf[1:])
        assert out[-1].data_ptr() % 16 == 4
    return out


def build_ln(c, ops, gen):
    M, C, eps = c["M"], c["C"], 1e-5
    x = NR.make_x(gen, M, 1, C, 1, const_group=False)
    gamma, beta = NR.make_affine(gen, C)
    gd, bd = _params(gamma, beta, c["align"])
    xd = x.reshape(M, C).cuda()

    def launch():
        o = Guarded(M, C, BF)
        ops.layernorm(xd, gd, bd, eps, out=o.view)
        return dict(y=o)

    def check(outs, keys):
        f = NR.forward(x, gamma, beta, 1, eps, 0, False)
        return dict(out=NR.check_elements(outs["y"].view.cpu().reshape(M, 1, C), f["y"], f["bnd"], "output"))

    return dict(launch=launch, check=check, acc=())


def build_lnact(c, ops, gen):
    M, C, eps, act = c["M"], c["C"], 1e-6, 2 if c["gelu"] else 0
    x = NR.make_x(gen, M, 1, C, 1, const_group=False)
    gamma, beta = NR.make_affine(gen, C)
    gd, bd, xd = gamma.cuda(), beta.cuda(), x.reshape(M, C).cuda()

    def launch():
        o = Guarded(M, C, BF)
        ops.layernorm_act(xd, gd, bd, eps, gelu=c["gelu"], out=o.view)
        return dict(y=o)

    def check(outs, keys):
        f = NR.forward(x, gamma, beta, 1, eps, act, False)
        return dict(out=NR.check_elements(outs["y"].view.cpu().reshape(M, 1, C), f["y"], f["bnd"], "output"))

    return dict(launch=launch, check=check, acc=())


def build_lnb(c, ops, gen):
    M, C, eps, acc, param = c["M"], c["C"], 1e-5, c["acc"], c["param"]
    x = NR.make_x(gen, M, 1, C, 1, const_group=False)
    gamma, _ = NR.make_affine(gen, C)
    dy = torch.randn(M, C, generator=gen).to(BF)
    old = torch.randn(M, C, generator=gen).to(BF)
    gd, xd, dyd, oldd = gamma.cuda(), x.reshape(M, C).cuda(), dy.cuda(), old.cuda()

    def launch():
        d = filled(M, C, oldd) if acc else Guarded(M, C, BF)
        dg, db = (vec(C), vec(C)) if param else (None, None)
        kw = dict(dx_into=d.view) if acc else dict(dx_out=d.view)
        if param:
            kw.update(dgamma_out=dg.vec, dbeta_out=db.vec)
        ops.layernorm_bwd(xd, gd, dyd, eps, want_param_grads=param, **kw)
        return dict(dx=d, dgamma=dg, dbeta=db)

    def check(outs, keys):
        b = NR.backward(x, gamma, torch.zeros(C), dy.reshape(M, 1, C), 1, eps, 0, False, old=old.reshape(M, 1, C) if acc else None)
        r = dict(out=NR.check_elements(outs["dx"].view.cpu().reshape(M, 1, C), b["dx"], b["bnd"], "dx"))
        if param:
            r["out"] = max(r["out"], NR.check_elements(outs["dgamma"].view.cpu()[0], b["dgamma"], b["bnd_dgamma"], "dgamma"),
                           NR.check_elements(outs["dbeta"].view.cpu()[0], b["dbeta"], b["bnd_dbeta"], "dbeta"))
        return r

    return dict(launch=launch, check=check, acc=("dx",) if acc else ())


def build_lnwin(c, ops, gen):
    B, H, W, C, ws, mode, eps = c["B"], c["H"], c["W"], c["C"], c["ws"], c["mode"], 1e-6
    img = NR.window_rows(B, H, W, ws)
    rows, n = img.numel(), B * H * W
    gamma, beta = NR.make_affine(gen, C)
    gd, bd = gamma.cuda(), beta.cuda()
    valid = img >= 0
    if mode == 1:
        x = NR.make_x(gen, n, 1, C, 1, const_group=False)
        xd = x.reshape(n, C).cuda()

        def launch():
            o = Guarded(rows, C, BF)
            ops.layernorm_window_partition(xd, gd, bd, eps, B, H, W, ws, out=o.view)
            return dict(y=o)

        def check(outs, keys):
            f = NR.forward(x, gamma, beta, 1, eps, 0, False)
            got = outs["y"].view.cpu()
            NR.check_pad_rows(got, ~valid)
            return dict(out=NR.check_elements(got[valid], f["y"].reshape(n, C)[img[valid]], f["bnd"].reshape(n, C)[img[valid]], "output"))
    else:
        win = NR.make_x(gen, rows, 1, C, 1, const_group=False).reshape(rows, C)
        sc = NR.make_x(gen, n, 1, C, 1, const_group=False).reshape(n, C)
        wd, sd = win.cuda(), sc.cuda()
        inv = torch.empty(n, dtype=torch.long)
        inv[img[valid]] = torch.arange(rows)[valid]

        def launch():
            o, xs = Guarded(n, C, BF), Guarded(n, C, BF)
            ops.window_merge_layernorm(wd, sd, gd, bd, eps, B, H, W, ws, out=o.view, xsum_out=xs.view)
            return dict(y=o, xsum=xs)

        def check(outs, keys):
            s64 = win[inv].to(NR.F64) + sc.to(NR.F64)
            xs = outs["xsum"].view.cpu()
            r1 = NR.check_elements(xs, s64, 2.0 ** -8 * s64.abs() + 1e-30, "xsum")
            f = NR.forward(xs.reshape(n, 1, C), gamma, beta, 1, eps, 0, False)
            return dict(out=max(r1, NR.check_elements(outs["y"].view.cpu().reshape(n, 1, C), f["y"], f["bnd"], "output")))

    return dict(launch=launch, check=check, acc=())


BUILD = dict(gn=build_gn, gnb=build_gnb, ln=build_ln, lnb=build_lnb, lnwin=build_lnwin, lnact=build_lnact)


# --------------------------------------------------------------------------------------------------- driver
def run_case(c, ops):
    gen = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    spec = BUILD[c["op"]](c, ops, gen)
    outs1, names = profiled(spec["launch"])
    names, keys = norm_keys(names)
    res = dict(id=c["id"], kernels=names, keys=sorted(set(keys)), ok=False, ratio=None, stat_ratio=None, guards=None, error=None)
    try:
        missing = [k for k in RC.expected_kernels(c["id"]) if k not in keys]
        if missing:
            raise CaseFailure(f"declared instantiation(s) not reached: {missing}")
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
            if left and name not in spec["acc"]:
                raise CaseFailure(f"{name}: {left} elements were never written")
        try:
            r = spec["check"](outs1, keys)
        except NR.BoundFailure as e:
            raise CaseFailure(str(e))
        res["ratio"], res["stat_ratio"], res["ok"] = r["out"], r.get("stat"), True
    except CaseFailure as e:
        res["error"] = str(e)
    return res


def conditioning(ops):
    """worst |rstd^ / rstd - 1| per route family and |mean| / sigma (B 2, C 320, 32 groups; slab HW 256, the others HW 4096)"""
    table = {}
    for route, HW, cs in (("slab", 256, False), ("three_launch", 4096, False), ("producer_statistics", 4096, True)):
        for ratio in SWEEP:
            c = dict(B=2, HW=HW, C=320, groups=32, C1=0, silu=False, cs=cs, stat=True)
            gen = torch.Generator().manual_seed(int(ratio) * 7 + HW)
            spec = build_gn(c, ops, gen, ratio=ratio)
            st = spec["launch"]()["stat"].view.cpu().to(NR.F64)
            m, r = NR.statistics(spec["x"], 32, spec["eps"])
            table.setdefault(route, {})[str(int(ratio))] = float((st[..., 1] / r - 1.0).abs().max())
    return table


def fmt(v):
    return f"{v:.3f}" if v is not None else "-"


def main():
    stray = sorted(k for k in os.environ if k.startswith("AE_") and k != "AE_LIB_PATH")
    if stray:
        print(f"norm_route_check: routing variables set: {stray} — the route cases run on the default plans only", flush=True)
        sys.exit(2)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from anyedit_amd import ops
    flt = sys.argv[1:]
    cases = [c for c in RC.NORM_CASES if not flt or any(f in c["id"] for f in flt)]
    results, t0 = [], time.time()
    aborted, cond = None, None
    for c in cases:
        t1 = time.time()
        try:
            r = run_case(c, ops)
        except Exception as e:   # a HIP / runtime error: start no further GPU work
            aborted = dict(id=c["id"], error=f"{type(e).__name__}: {e}")
            print(f"ABORT {c['id']}: {aborted['error']}", flush=True)
            break
        results.append(r)
        print(f"{'PASS' if r['ok'] else 'FAIL'} {r['id']:30s} {time.time() - t1:5.1f}s output {fmt(r['ratio']):>6s} statistics {fmt(r['stat_ratio']):>6s} "
              f"guards {r['guards']} kernels {r['keys'] or r['kernels']}" + (f"  ERROR {r['error']}" if r["error"] else ""), flush=True)
    if aborted is None and not flt:
        try:
            cond = conditioning(ops)
            print("CONDITIONING " + json.dumps(cond), flush=True)
        except Exception as e:
            aborted = dict(id="conditioning sweep", error=f"{type(e).__name__}: {e}")
            print(f"ABORT conditioning sweep: {aborted['error']}", flush=True)
    summary = dict(results=results, aborted=aborted, conditioning=cond, seconds=round(time.time() - t0, 1))
    print("NORM_ROUTE_SUMMARY " + json.dumps(summary), flush=True)
    sys.exit(0 if aborted is None and all(r["ok"] for r in results) else 1)


if __name__ == "__main__":
    main()
