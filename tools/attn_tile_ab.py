#!/usr/bin/env python3
"""A/B probe for the streaming 64-key-tile attention kernels (attn_kernel of attention.hip, attn_mutual_kernel of masactrl.hip; csrc/attn_tile.hpp).

  python tools/attn_tile_ab.py                  # bits: one line per case, "<case> <sha1 of the output bits>" (or NONFINITE)
  python tools/attn_tile_ab.py --time           # the same launch forms at 2048 tokens: "<case> <median us> <min> <max>" over 5 windows of 10 launches
  python tools/attn_tile_ab.py --compare A B    # two saved outputs of the first form: every case must carry the same hash in both
  python tools/attn_tile_ab.py [--time] --groups w8_occ4,w8_occ0    # only these knob environments

attention.hip reads its tuning knobs once per process, so the cases are grouped by environment (tests/route_cases.py, ATTN_GENERAL_ENVS) and every
group runs in a fresh child process with exactly its variables set.  The library is the one AE_LIB_PATH names, or the product library:
    AE_LIB_PATH=anyedit_amd/libanyedit_hip_parent.so python tools/attn_tile_ab.py > parent.txt ; python tools/attn_tile_ab.py > new.txt
The last lines of the bits run compare, inside ONE library, ops.attention_mutual (identity remap, no classes) with ops.attention on the same
packed operands at head dim 64: "mutual-vs-general ... equal" is what tests/test_hip_masactrl.py asserts."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ENVS = {"default": {}, "nofast": {"AE_ATTN_FAST": "0"}, "w8": {"AE_ATTN_FAST": "0", "AE_ATTN_W8": "1"},
        "w8_occ4": {"AE_ATTN_FAST": "0", "AE_ATTN_W8": "1", "AE_ATTN_SAM_OCC": "4"}, "w8_occ0": {"AE_ATTN_FAST": "0", "AE_ATTN_W8": "1", "AE_ATTN_SAM_OCC": "0"},
        "shortk": {"AE_ATTN_FAST": "0", "AE_ATTN_SHORTK_QF1": "1"}}
KNOBS = ("AE_ATTN_FAST", "AE_ATTN_W8", "AE_ATTN_SHORTK_QF1", "AE_ATTN_QF40", "AE_ATTN_SAM_OCC")
SEQ = ((1, 1), (63, 63), (64, 64), (65, 65), (129, 129), (300, 300), (300, 77))
B, H = 2, 2


def general(ops, torch, D, Nq, Nk, form, seed, Bh=(B, H)):
    """one ops.attention launch on packed seeded operands; returns the tensors whose bits count"""
    b, h = Bh
    gen = torch.Generator().manual_seed(seed)
    inner = h * D
    q = torch.randn(b * Nq, inner, generator=gen).bfloat16().cuda()
    kv = torch.randn(b * Nk, 2 * inner, generator=gen).bfloat16().cuda()
    qs, ks = (Nq * inner, D, inner), (Nk * 2 * inner, D, 2 * inner)
    kw, outs = {}, []
    if form == "mask":
        m = (torch.rand(b, Nk, generator=gen) < 0.7).to(torch.uint8)
        m[:, 0] = 1
        kw["key_mask"] = m.cuda()
    elif form.startswith("rel"):
        kH, kW = (int(x) for x in form[3:].split("x"))
        assert kH * kW == Nk
        kw.update(rel_h=torch.randn(b * h, Nq, kH, generator=gen).cuda(), rel_w=torch.randn(b * h, Nq, kW, generator=gen).cuda(), kH=kH, kW=kW)
    elif form.startswith("seg"):
        Nk2 = int(form[3:])
        kv2 = torch.randn(b * Nk2, 2 * inner, generator=gen).bfloat16().cuda()
        kw["seg2"] = (kv2, kv2[:, inner:], Nk2, (Nk2 * 2 * inner, D, 2 * inner), (Nk2 * 2 * inner, D, 2 * inner), torch.rand(b, generator=gen).cuda())
        if form.endswith("77"):
            kw["lse"], kw["lse2"] = torch.empty(b, h, Nq).cuda(), torch.empty(b, h, Nq).cuda()
            outs += [kw["lse"], kw["lse2"]]
    elif form == "accum":
        kw.update(out=torch.randn(b, Nq, inner, generator=gen).bfloat16().cuda(), accumulate=True, out_scale=torch.rand(b, generator=gen).cuda())
    elif form == "lse":
        kw["lse"] = torch.empty(b, h, Nq).cuda()
        outs.append(kw["lse"])
    out = ops.attention(q, kv, kv[:, inner:], b, h, Nq, Nk, D, D ** -0.5, qs, ks, ks, **kw)
    return [out] + outs, lambda: ops.attention(q, kv, kv[:, inner:], b, h, Nq, Nk, D, D ** -0.5, qs, ks, ks, **kw)


def digest(torch, tensors):
    torch.cuda.synchronize()
    hsh = hashlib.sha1()
    for t in tensors:
        if not bool(torch.isfinite(t.float()).all()):
            return "NONFINITE"
        hsh.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return hsh.hexdigest()


def bits_cases(group):
    """(name, D, Nq, Nk, form) of the group's launches of ops.attention"""
    dims = {"default": (8, 48, 64, 128), "nofast": (40, 160), "w8": (80,), "w8_occ4": ()}[group]
    cases = [(D, nq, nk, "plain") for D in dims for nq, nk in SEQ]
    if group == "default":
        cases += [(64, 300, 77, "mask"), (64, 129, 129, "mask"), (64, 77, 65, "rel5x13"), (64, 77, 80, "rel2x40"), (64, 77, 128, "rel2x64")]
    if group == "nofast":
        cases += [(40, 300, 77, "mask"), (40, 129, 129, "mask"), (40, 300, 77, "seg1"), (40, 129, 129, "seg77"), (40, 300, 77, "accum"), (40, 65, 65, "lse"),
                  (40, 1088, 1088, "plain")]
    if group == "w8":
        cases += [(80, 300, 77, "mask"), (80, 129, 129, "seg77")]
    if group in ("nofast", "w8", "w8_occ4"):   # the rel-pos forms at d = 40 / 80: row tiles (2 x 64, 3 x 64) and LDS tables (5 x 13)
        cases += [(D, 77, nk, f) for D in (40, 80) for nk, f in ((128, "rel2x64"), (192, "rel3x64"), (65, "rel5x13"))]
    return cases


def mutual_bits(ops, torch):
    import test_hip_masactrl as TM
    import masactrl_ref as R
    lines = []

    def run(name, Bm, N, D, src, qcls=None, kcls=None, kcnt=None, seed=0):
        buf, st, _ = TM._packed_operands(Bm, 2, N, D, seed)
        dev, inner = buf.cuda(), 2 * D
        if qcls is not None and kcnt is None:
            kcnt = torch.stack([(kcls == 0).sum(1), (kcls == 1).sum(1)], 1).to(torch.int32)
        c = [None if x is None else x.cuda() for x in (qcls, kcls, kcnt)]
        out = ops.attention_mutual(dev, dev[:, inner:], dev[:, 2 * inner:], Bm, 2, N, D, D ** -0.5, st, st, st, src, qcls=c[0], kcls=c[1], kcnt=c[2])
        lines.append(f"mutual {name} D={D} N={N} {digest(torch, [out])}")

    for D in (40, 64, 80, 160):
        for N in TM.REMAP_N:
            run("halves", 4, N, D, (0, 0, 2, 2), seed=10 * D + N)
            gen = torch.Generator().manual_seed(100 + N + D)
            run("random", 6, N, D, [int(s) for s in torch.randint(0, 6, (6,), generator=gen)], seed=10 * D + N + 1)
        for kind, N in TM.CLASS_CASES:
            qcls, kcls = TM._class_pattern(kind, N, torch.Generator().manual_seed(7 * N + D))
            run("classes-" + kind, 4, N, D, (0, 0, 2, 2), qcls, kcls, seed=3 * N + D)
        N = 36   # the empty-class case: the unconditional half's source has no foreground key, the conditional half's one background key
        gen = torch.Generator().manual_seed(50 + D)
        kcls = torch.zeros(4, N, dtype=torch.uint8)
        kcls[2] = 1
        kcls[2, 5] = 0
        kcnt = torch.tensor([[N, 0], [0, 0], [1, N - 1], [0, 0]], dtype=torch.int32)
        qcls = torch.full((4, N), R.CLS_ANY, dtype=torch.uint8)
        qcls[1], qcls[3] = torch.randint(0, 2, (N,), generator=gen).to(torch.uint8), torch.randint(0, 2, (N,), generator=gen).to(torch.uint8)
        run("empty-class", 4, N, D, (0, 0, 2, 2), qcls, kcls, kcnt, seed=6 + D)
    for N in (1, 65, 300):   # the two kernels on one core: identity remap, no classes, against the general kernel at head dim 64
        lines.append(f"mutual-vs-general (same library) D=64 N={N} {'equal' if mutual_vs_general(ops, torch, 64, N) else 'UNEQUAL'}")
    return lines


def time_cases(group):
    dims = {"default": (8, 16, 32, 48, 64, 96, 128), "nofast": (40, 80, 160), "shortk": (40, 80, 160)}.get(group, (40, 80))
    nk = 128 if group == "shortk" else 2048
    forms = ("plain", "mask", f"seg{nk}") + (() if group == "shortk" else ("rel32x32", "rel16x128", "rel32x64"))
    return [(D, 2048, (1024 if f == "rel32x32" else nk), f) for D in dims for f in forms]


def mutual_vs_general(ops, torch, D, N):
    """identity remap, no classes, against ops.attention on the same packed operands, inside this process's library"""
    import test_hip_masactrl as TM
    buf, st, _ = TM._packed_operands(2, 2, N, D, D + N)
    dev, inner = buf.cuda(), 2 * D
    a = ops.attention_mutual(dev, dev[:, inner:], dev[:, 2 * inner:], 2, 2, N, D, D ** -0.5, st, st, st, (0, 1))
    g = ops.attention(dev, dev[:, inner:], dev[:, 2 * inner:], 2, 2, N, N, D, D ** -0.5, st, st, st)
    torch.cuda.synchronize()
    return bool(torch.isfinite(g.float()).all()) and torch.equal(a, g)


def time_mutual(ops, torch):
    """ops.attention_mutual at 2048 tokens, B = 4, H = 8, src (0, 0, 2, 2), without and with classes: one entry per attn_mutual_kernel instantiation"""
    B_, H_, N = 4, 8, 2048
    for D in (40, 64, 80, 160):
        gen = torch.Generator().manual_seed(D)
        inner = H_ * D
        qkv = torch.randn(B_ * N, 3 * inner, generator=gen).bfloat16().cuda()
        st = (N * 3 * inner, D, 3 * inner)
        kc = torch.randint(0, 2, (B_, N), generator=gen).to(torch.uint8)
        qc = torch.randint(0, 2, (B_, N), generator=gen).to(torch.uint8)
        cnt = torch.stack([(kc == 0).sum(1), (kc == 1).sum(1)], 1).to(torch.int32)
        out = torch.empty(B_, N, inner, dtype=torch.bfloat16, device="cuda")
        for name, kw in (("plain", {}), ("classes", dict(qcls=qc.cuda(), kcls=kc.cuda(), kcnt=cnt.cuda()))):
            yield f"mutual D={D} N={N} {name}", (lambda kw=kw, D=D, qkv=qkv, st=st, out=out, inner=inner: ops.attention_mutual(
                qkv, qkv[:, inner:], qkv[:, 2 * inner:], B_, H_, N, D, D ** -0.5, st, st, st, (0, 0, 2, 2), out=out, **kw))


def window_us(torch, fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10):
            fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 100.0)
    return f"{statistics.median(t):.1f} {min(t):.1f} {max(t):.1f}"


def child(group, timing):
    import torch
    from anyedit_amd import ops
    from anyedit_amd._lib import AnyEditHipError
    if timing:
        for D, Nq, Nk, form in time_cases(group):
            name = f"{group} D={D} Nq={Nq} Nk={Nk} {form}"
            try:
                _, fn = general(ops, torch, D, Nq, Nk, form, D + Nk, Bh=(2, 8))
            except (AnyEditHipError, ValueError):
                print(f"{name} unsupported")
                continue
            print(f"{name} " + window_us(torch, fn))
        if group == "default":
            for name, fn in time_mutual(ops, torch):
                print(f"{name} " + window_us(torch, fn))
        return
    for D, Nq, Nk, form in bits_cases(group):
        outs, _ = general(ops, torch, D, Nq, Nk, form, 1000 * D + 10 * Nq + Nk)
        print(f"{group} D={D} Nq={Nq} Nk={Nk} {form} {digest(torch, outs)}")
    if group == "default":
        print("\n".join(mutual_bits(ops, torch)))


def compare(a, b):
    rows = [dict(l.rsplit(" ", 1) for l in open(p).read().splitlines() if l.strip()) for p in (a, b)]
    bad = [k for k in rows[0] if rows[0][k] != rows[1].get(k) or rows[0][k] in ("NONFINITE", "UNEQUAL")]
    bad += [k for k in rows[1] if k not in rows[0]]
    for k in rows[0]:
        if not k.startswith("mutual-vs-general"):
            print(f"{k}: {'new vs parent equal' if k not in bad else 'UNEQUAL OR NON-FINITE'}")
    print(f"{len(rows[0])} cases, {len(bad)} unequal or non-finite")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--group", default=None)
    ap.add_argument("--groups", default=None, help="comma-separated environments to run (default: all the mode uses)")
    ap.add_argument("--compare", nargs=2, default=None)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if a.group:
        return child(a.group, a.time)
    for group in (a.groups.split(",") if a.groups else ENVS if a.time else ("default", "nofast", "w8", "w8_occ4")):
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(ENVS[group])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--group", group] + (["--time"] if a.time else []), env=env, timeout=600)
        if r.returncode != 0:
            sys.exit(f"group {group} failed with exit status {r.returncode}")


if __name__ == "__main__":
    main()
