"""Route cases of attention.hip on the GPU: which attn_kernel<D, QF, NW, DBUF, BIAS, HAS_MASK, SEG2, OCC4> ran, and is every output element right.

The sibling of tools/route_check.py (whose guarded buffers, profiler capture, kernel-name keys, bound check and float64 attention reference it
uses) for ATTN_GENERAL_CASES of tests/route_cases.py.  One process per environment of ATTN_GENERAL_ENVS: tests/test_kernel_routes.py starts it
with every AE_* variable removed and exactly that environment's set (attention.hip reads its tuning knobs once per process).  For each case:
  1. seeded bf16 operands in the case's layout ("qkv": fused [B N, 3 H D] rows for self-attention, q rows + packed kv rows otherwise; "bhnd"),
     a key mask [B, Nk] that differs between the samples, rel_h ~ N(0, 1) and rel_w ~ U(-2, 1) (two distributions: a swap fails), a gate of
     both signs; the op runs through `ops.attention` once under torch.profiler -> the kernel names of the case, which must include every
     instantiation whose ATTN_GENERAL_LEDGER row lists the case;
  2. out ([B Nq, H D] with row stride H D + o_pad), lse and lse2 are views inside sentinel-filled allocations: the guard areas and the pad
     columns must be unchanged, no sentinel may be left inside (an accumulate target is pre-filled with a seeded bf16 tensor instead), and a
     second run on fresh buffers must be bit-identical;
  3. EVERY element of every (batch, head) is compared with float64 on the same bf16 operands (route_check.attn_segment_ref: masked_fill(-finfo.max)
     then softmax, so a sample with no live key gives the plain mean of its Nk value rows).

Bounds (derived in the docstring of tools/route_check.py; nothing is added here).  Output: |err| <= 2^-8 |ref| + 2^-8 sum_j p_j |v_j|
(+ 2^-9 (max|rel_h| + max|rel_w|) (sum_j p_j |v_j| + |ref|) with a rel-pos bias) + 1e-30; with a gate g and an accumulate target prev, the stored
value is prev + g r: 2^-8 |prev + g r| + |g| (the probability terms of r) + 1e-30 — one rounding of the stored sum and one of each probability.
With a second segment r = r1 + scale2 r2 and the probability terms add the same way.  Log-sum-exp: that docstring's bound unchanged, the maximum
over the live keys only; lse and lse2 are both compared.  Where a sample has no live key `lse` must still be fully written, and is not compared:
the kernel defines no value for it there.

    python tools/attn_general_route_check.py --env NAME [case-id-substring ...]   # one line per case (ratio, lse_ratio), then `ATTN_GENERAL_SUMMARY {json}`
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
from route_check import BF, F64, CaseFailure, Guarded, attn_out_bound, attn_segment_ref, bound_check, profiled, rnd, route_keys  # noqa: E402

F32 = torch.float32
FAMILIES = re.compile(r"\b(attn_kernel)<([^<>]*)>")      # \b: not fp8_attn_kernel; attn_fast_kernel / attn_pipe_kernel are other names
GATES = (0.75, -1.25)


def key_mask(kind, B, Nk, gen):
    """live [B, Nk] bool (False = removed); sample 1 always differs from sample 0"""
    live = torch.ones(B, Nk, dtype=torch.bool)
    rand = lambda: torch.rand(Nk, generator=gen) < 0.5
    if kind == "rand":
        for b in range(B):
            live[b] = rand()
            live[b, int(torch.randint(0, Nk, (1,), generator=gen))] = True
    elif kind == "lead":
        live[:, :64] = False
        if Nk >= 66:
            live[1:, min(69, Nk - 2)] = False
        else:                       # one live key behind the dead tile: sample 1 keeps key 63 as well
            live[1:, 63] = True
    elif kind == "trail":
        t = (Nk - 1) // 64 - 1 if Nk % 64 else Nk // 64 - 1
        live[:, 64 * t:64 * t + 64] = False
        live[1:, 3] = False
    elif kind == "tailkey":
        assert Nk % 64
        live[:, Nk // 64 * 64 + (Nk % 64) // 2] = False
        live[1:, Nk - 1] = False
    elif kind == "all":
        live[0] = False
        for b in range(1, B):
            live[b] = rand()
            live[b, 0] = True
    else:
        raise ValueError(kind)
    return live


def build(c, ops, gen):
    B, H, Nq, Nk, D = c["B"], c["H"], c["Nq"], c["Nk"], c["D"]
    C, scale = H * D, D ** -0.5
    nk2, rel, mask, gate, onto, o_pad = c.get("nk2"), c.get("rel"), c.get("mask"), c.get("gate"), c.get("onto"), c.get("o_pad", 0)
    if c["lay"] == "qkv" and Nq == Nk and not nk2:       # self-attention on fused qkv rows [B N, 3C]
        qkv = rnd(gen, B * Nq, 3 * C)
        q = k = v = qkv
        qs = ks = vs = (Nq * 3 * C, D, 3 * C)
        off = (0, C, 2 * C)
        qc = qkv.cuda()
        dq, dk, dv = qc, qc[:, C:], qc[:, 2 * C:]
    elif c["lay"] == "qkv":                              # q rows [B Nq, C] + packed kv rows [B Nk, 2C]
        q, kv = rnd(gen, B * Nq, C), rnd(gen, B * Nk, 2 * C)
        k = v = kv
        qs, ks = (Nq * C, D, C), (Nk * 2 * C, D, 2 * C)
        vs, off = ks, (0, 0, C)
        kvc = kv.cuda()
        dq, dk, dv = q.cuda(), kvc, kvc[:, C:]
    else:
        q, k, v = rnd(gen, B * H, Nq, D), rnd(gen, B * H, Nk, D), rnd(gen, B * H, Nk, D)
        qs, ks, vs = (H * Nq * D, Nq * D, D), (H * Nk * D, Nk * D, D), (H * Nk * D, Nk * D, D)
        off = (0, 0, 0)
        dq, dk, dv = q.cuda(), k.cuda(), v.cuda()

    def view4(t, n, st, o):   # (B, H, n, D) float64 view of a strided operand
        return t.as_strided((B, H, n, D), st + (1,), o).to(F64)

    Q4, K4, V4 = view4(q, Nq, qs, off[0]), view4(k, Nk, ks, off[1]), view4(v, Nk, vs, off[2])
    seg = K2 = V2 = s2 = None
    if nk2:
        k2 = rnd(gen, B * nk2, 2 * C)
        st2 = (nk2 * 2 * C, D, 2 * C)
        s2 = torch.linspace(0.5, 1.5, B)
        k2c = k2.cuda()
        seg = (k2c, k2c[:, C:], nk2, st2, st2, s2.cuda())
        K2, V2 = view4(k2, nk2, st2, 0), view4(k2, nk2, st2, C)
    relh = relw = None
    if rel:
        relh = torch.randn(B * H, Nq, rel[0], generator=gen)
        relw = torch.rand(B * H, Nq, rel[1], generator=gen) * 3.0 - 2.0
    live = key_mask(mask, B, Nk, gen) if mask else None
    g = torch.tensor(GATES[:B], dtype=F32) if gate else None
    prev = rnd(gen, B * Nq, C) if onto else None
    dev = dict(relh=relh.cuda() if rel else None, relw=relw.cuda() if rel else None, mask=live.to(torch.uint8).cuda() if mask else None,
               gate=g.cuda() if gate else None, prev=prev.cuda() if onto else None)
    ld = C + o_pad

    def launch():
        o = Guarded(B * Nq, C, BF, ld=ld)
        if onto:
            o.view.copy_(dev["prev"])
        outs = dict(out=o, lse=Guarded(1, B * H * Nq, F32, guard=4096))
        if nk2:
            outs["lse2"] = Guarded(1, B * H * Nq, F32, guard=4096)
        ops.attention(dq, dk, dv, B, H, Nq, Nk, D, scale, qs, ks, vs, out=o.view, rel_h=dev["relh"], rel_w=dev["relw"], kH=rel[0] if rel else 0,
                      kW=rel[1] if rel else 0, key_mask=dev["mask"], out_scale=dev["gate"], accumulate=bool(onto), seg2=seg,
                      lse=outs["lse"].view.reshape(B, H, Nq), lse2=outs["lse2"].view.reshape(B, H, Nq) if nk2 else None, o_strides=(Nq * ld, D, ld))
        return outs

    def check(outs):
        got = outs["out"].view.cpu().reshape(B, Nq, H, D)
        lse = {n: outs[n].view.cpu().reshape(B, H, Nq) for n in outs if n != "out"}
        ratio, lse_ratio = 0.0, 0.0
        for b in range(B):
            for h in range(H):
                bh = b * H + h
                bias = (relh[bh].to(F64), relw[bh].to(F64)) if rel else None
                s1 = attn_segment_ref(Q4[b, h], K4[b, h], V4[b, h], scale, bias=bias, live=live[b] if mask else None)
                r, sv, lrefs = s1["r"], s1["sv"], [("lse", s1)]
                if nk2:
                    sg = attn_segment_ref(Q4[b, h], K2[b, h], V2[b, h], scale)
                    r, sv = r + float(s2[b]) * sg["r"], sv + float(s2[b]) * sg["sv"]
                    lrefs.append(("lse2", sg))
                gb = float(g[b]) if gate else 1.0
                stored = gb * r + (prev.reshape(B, Nq, H, D)[b, :, h].to(F64) if onto else 0.0)
                bnd = attn_out_bound(r, sv, s1["bmax"], stored=stored, gate=gb)
                ratio = max(ratio, bound_check(got[b, :, h], stored, bnd, f"output (batch {b}, head {h})"))
                for name, s in lrefs:
                    if s["L2"] is None:      # no live key: written (checked by the caller), value undefined
                        continue
                    lse_ratio = max(lse_ratio, bound_check(lse[name][b, h][:, None], s["L2"][:, None], s["L2_bnd"][:, None], f"{name} (batch {b}, head {h})"))
        return ratio, lse_ratio

    return dict(launch=launch, check=check)


def run_case(c, ops):
    gen = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    spec = build(c, ops, gen)
    res = dict(id=c["id"], kernels=[], keys=[], ok=False, ratio=None, lse_ratio=None, guards=None, error=None)
    try:
        outs1, names = profiled(spec["launch"])
        names, keys = route_keys(names, FAMILIES)
        res["kernels"], res["keys"] = names, sorted(set(keys))
        missing = [k for k in RC.attn_general_expected(c["id"]) if k not in keys]
        if missing:
            raise CaseFailure(f"declared instantiation(s) not reached: {missing}")
        outs2 = spec["launch"]()
        torch.cuda.synchronize()
        gd = all(g.guards_intact() for o in (outs1, outs2) for g in o.values())
        res["guards"] = "intact" if gd else "CLOBBERED"
        if not gd:
            raise CaseFailure("a guard area or a pad column was written")
        for name, g in outs1.items():
            if not torch.equal(g.bits(), outs2[name].bits()):
                raise CaseFailure(f"{name}: two runs differ")
            left = int((g.bits() == g.sent).sum())
            if left:
                raise CaseFailure(f"{name}: {left} elements were never written")
        res["ratio"], res["lse_ratio"] = spec["check"](outs1)
        res["ok"] = True
    except CaseFailure as e:
        res["error"] = str(e)
    return res


def main():
    args = sys.argv[1:]
    if len(args) < 2 or args[0] != "--env" or args[1] not in RC.ATTN_GENERAL_ENVS:
        print(__doc__.strip().splitlines()[-1], flush=True)
        sys.exit(2)
    env, flt = args[1], args[2:]
    want = RC.ATTN_GENERAL_ENVS[env]
    have = {k: v for k, v in os.environ.items() if k.startswith("AE_") and k != "AE_LIB_PATH"}
    if have != want:
        print(f"attn_general_route_check: --env {env} runs with the AE_* variables {want}, got {have}", flush=True)
        sys.exit(2)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from anyedit_amd import ops
    cases = [c for c in RC.ATTN_GENERAL_CASES if c["env"] == env and (not flt or any(f in c["id"] for f in flt))]
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
        fmt = lambda x: "-" if x is None else f"{x:.3f}"
        print(f"{'PASS' if r['ok'] else 'FAIL'} {r['id']:40s} {time.time() - t1:5.2f}s ratio {fmt(r['ratio'])} lse_ratio {fmt(r['lse_ratio'])} guards {r['guards']} "
              f"kernels {r['keys'] or r['kernels']}" + (f"  ERROR {r['error']}" if r["error"] else ""), flush=True)
    byid = {r["id"]: r for r in results}
    per_kernel = {}
    for key, row in RC.ATTN_GENERAL_LEDGER.items():
        done = [byid[i] for i in row[-1] if i in byid and byid[i]["ratio"] is not None]
        if done:
            per_kernel[key] = [max(r["ratio"] for r in done), max(r["lse_ratio"] for r in done)]
            print(f"worst error / bound  {key:56s} output {per_kernel[key][0]:.3f} lse {per_kernel[key][1]:.3f}  ({len(done)} cases)", flush=True)
    summary = dict(env=env, results=results, aborted=aborted, per_kernel=per_kernel, seconds=round(time.time() - t0, 1))
    print("ATTN_GENERAL_SUMMARY " + json.dumps(summary), flush=True)
    sys.exit(0 if aborted is None and all(r["ok"] for r in results) else 1)


if __name__ == "__main__":
    main()
