"""Route ledger of gemm_conv.hip / attention_fast.hip / norm.hip / gemm_rowpanel.hip / ff_fused.hip / attention.hip (tests/route_cases.py) and
the GPU route cases behind it.

CPU: the set of kernel instantiations the default build compiles — hipcc's device-only LLVM IR of the six sources with the library's flags
(at -O0: which kernels a translation unit emits does not depend on the optimisation level) — must equal the ledger's keys, in both
directions, so an instantiation that is added or removed fails here until someone classifies it.

GPU: tools/route_check.py in a fresh child process with every AE_* variable removed from its environment (this test session itself runs
with AE_ROWPANEL_ANY_M=1, set by test_hip_ops.py): every case must reach its declared instantiations, pass the element-wise float64
check, leave its guard areas untouched and repeat bit for bit; every `default` ledger row must be reached by each case it lists.  Every
attention case also carries the log-sum-exp outputs through the same checks and reports their worst error / bound as `lse_ratio`.
The cases of norm.hip run the same way in a child process of their own (tools/norm_route_check.py, test_norm_route_cases_on_gpu).
The cases of gemm_rowpanel.hip / ff_fused.hip (tools/rowpanel_route_check.py, test_rowpanel_route_cases_on_gpu) take two children: the
small ones reach the kernels through the library's test hook, AE_ROWPANEL_ANY_M=1 in that child's environment only; the plan threshold
(192 blocks of 192 rows run the kernels, 191 run the tiled gemm_kernel) is crossed from both sides with every AE_* variable removed.
The cases of attention.hip's general attn_kernel (tools/attn_general_route_check.py, test_attn_general_route_cases_on_gpu) take one child per
environment of route_cases.ATTN_GENERAL_ENVS, one after another: the `default` rows with every AE_* variable removed, each `env` row with
exactly its row's variables set (attention.hip reads those tuning knobs once per process).
"""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import route_cases as RC  # noqa: E402

NORM_FAMILIES = ("gn_slab_kernel", "gn_apply_kernel", "gnb_slab_kernel", "layernorm_rows_kernel", "layernorm_kernel", "layernorm_window_kernel",
                 "layernorm_narrow_kernel", "layernorm_bwd_kernel")
ROWPANEL_FAMILIES = ("gemm_rowpanel_kernel", "ff_fused_kernel")
FAMILY_RE = re.compile(r"^void (?:\(anonymous namespace\)::)?(gemm_kernel|attn_fast_kernel|attn_pipe_kernel|attn_kernel|" + "|".join(NORM_FAMILIES + ROWPANEL_FAMILIES) + r")<([^<>]*)>\(")
NORM_PLAIN = ("gn_stats_kernel", "gn_finalize_kernel", "gn_finalize_cs_kernel", "gnb_partial_kernel", "gnb_finalize_kernel", "gnb_apply_kernel",
              "layernorm_param_grad_kernel")
PLAIN = ("splitk_reduce_kernel", "colstats_kernel") + NORM_PLAIN
ROWPANEL_CHILD_TIMEOUT = 120    # seconds for each child of tools/rowpanel_route_check.py; measured on the MI355X: 5.1 s (hook, 45 cases) and 8.8 s (default, 4 cases at M = 36673)
ATTN_GENERAL_CHILD_TIMEOUT = 60    # seconds for each child of tools/attn_general_route_check.py; measured on the MI355X, whole children: 5.5 s (default,
                                   # 209 cases), 4.3 s (nofast, 35), 4.1 s (w8, 26), 3.7 s (w8_occ4, 4), 3.8 s (w8_occ0, 8), 4.3 s (shortk, 36): 26 s for the six
NORM_CHILD_TIMEOUT = 180    # seconds for tools/norm_route_check.py; measured on the MI355X: 12 s for the whole child (8.8 s of cases and sweep)


def _kernel_keys(ir_text):
    mangled = re.findall(r"^define\b[^@\n]*\bamdgpu_kernel\b[^@\n]*@(\S+?)\(", ir_text, re.M)
    dm = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    keys = []
    for name in dm[:len(mangled)]:
        m = FAMILY_RE.match(name)
        if m:
            keys.append(f"{m.group(1)}<{', '.join(x.strip() for x in m.group(2).split(','))}>")
        else:
            keys += [p for p in PLAIN if re.search(r"::" + p + r"\(|^" + p + r"\(", name)]
    return keys


def compiled_instantiations(tmpdir):
    from anyedit_amd import build as B
    hipcc = B._hipcc()
    keys = []
    for src in ("gemm_conv.hip", "attention_fast.hip", "norm.hip", "gemm_rowpanel.hip", "ff_fused.hip", "attention.hip"):
        flags = [("-O0" if f == "-O3" else f) for f in B.FLAGS if f != "-fPIC"] + B.EXTRA.get(src, [])
        out = os.path.join(str(tmpdir), src.replace(".hip", ".ll"))
        subprocess.run([hipcc] + flags + ["--cuda-device-only", "-emit-llvm", "-S", os.path.join(B.CSRC, src), "-o", out], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        with open(out) as f:
            keys += _kernel_keys(f.read())
    return keys


def test_ledger_rows_are_well_formed():
    ids = set(RC.CASE_IDS)
    assert len(ids) == len(RC.CASES), "duplicate case ids"
    for key, row in RC.LEDGER.items():
        kind, what = row
        assert kind == "default", (key, kind)
        assert what and all(c in ids for c in what), (key, [c for c in what if c not in ids])
    for c in RC.CASES:
        assert c["op"] in ("conv", "up2", "gemm", "ln", "attn"), c
    # every case asserts a route: it appears in at least one `default` row
    listed = {c for kind, what in RC.LEDGER.values() if kind == "default" for c in what}
    assert not ids - listed, f"cases that assert no route: {sorted(ids - listed)}"
    # every attention row is reached by at least one case whose last 128-query block is ragged
    nq = {c["id"]: c["Nq"] for c in RC.CASES if c["op"] == "attn"}
    whole = [k for k, (kind, what) in RC.LEDGER.items() if kind == "default" and k.startswith("attn_") and all(nq[c] % 128 == 0 for c in what)]
    assert not whole, f"attention rows reached only at Nq % 128 == 0: {whole}"


def test_norm_ledger_rows_are_well_formed():
    ids = set(RC.NORM_CASE_IDS)
    assert len(ids) == len(RC.NORM_CASES) and not ids & set(RC.CASE_IDS), "duplicate case ids"
    assert not set(RC.NORM_LEDGER) & set(RC.LEDGER)
    for key, (kind, what) in RC.NORM_LEDGER.items():
        assert kind == "default", (key, kind)
        assert what and all(c in ids for c in what), (key, [c for c in what if c not in ids])
    for c in RC.NORM_CASES:
        assert c["op"] in ("gn", "gnb", "ln", "lnb", "lnwin", "lnact"), c
    listed = {c for kind, what in RC.NORM_LEDGER.values() for c in what}
    assert not ids - listed, f"cases that assert no route: {sorted(ids - listed)}"
    # every group pack wider than one group is reached by a concat input whose split falls inside a pack (C1 % (GP * cpg) != 0)
    byid = {c["id"]: c for c in RC.NORM_CASES}
    for key, (kind, what) in RC.NORM_LEDGER.items():
        m = re.match(r"gnb?_slab_kernel<\d+, ([24])\b", key)
        if m:
            gp = int(m.group(1))
            assert any(byid[c]["C1"] and byid[c]["C1"] % (gp * byid[c]["C"] // byid[c]["groups"]) for c in what), f"{key}: no case with a concat split inside a pack"


def test_attn_general_ledger_rows_are_well_formed():
    ids = set(RC.ATTN_GENERAL_CASE_IDS)
    others = set(RC.CASE_IDS) | set(RC.NORM_CASE_IDS) | set(RC.ROWPANEL_CASE_IDS)
    assert len(ids) == len(RC.ATTN_GENERAL_CASES) and not ids & others, "duplicate case ids"
    assert not set(RC.ATTN_GENERAL_LEDGER) & (set(RC.LEDGER) | set(RC.NORM_LEDGER) | set(RC.ROWPANEL_LEDGER))
    # only this ledger has `env` rows: every row of the others is reached with no AE_* variable set
    for led in (RC.LEDGER, RC.NORM_LEDGER, RC.ROWPANEL_LEDGER):
        assert all(len(row) == 2 and row[0] == "default" for row in led.values())
    byid = {c["id"]: c for c in RC.ATTN_GENERAL_CASES}
    knobs = ("AE_ATTN_FAST", "AE_ATTN_W8", "AE_ATTN_SHORTK_QF1", "AE_ATTN_QF40", "AE_ATTN_SAM_OCC")
    assert RC.ATTN_GENERAL_ENVS["default"] == {} and all(set(e) <= set(knobs) for e in RC.ATTN_GENERAL_ENVS.values())
    for key, row in RC.ATTN_GENERAL_LEDGER.items():
        assert re.fullmatch(r"attn_kernel<\d+, [124], [48], (true|false), [012], (true|false), (true|false), (true|false)>", key), key
        assert (row[0] == "default" and len(row) == 2) or (row[0] == "env" and len(row) == 3 and row[1] and row[1] in RC.ATTN_GENERAL_ENVS.values()), (key, row)
        what = row[-1]
        assert what and all(c in ids for c in what), (key, [c for c in what if c not in ids])
        # a case runs in the environment of the row that lists it, and the row is the instantiation the case declares
        want_env = {} if row[0] == "default" else row[1]
        assert all(RC.ATTN_GENERAL_ENVS[byid[c]["env"]] == want_env and RC.attn_general_key(byid[c]) == key for c in what), key
        # every row is reached by at least one case whose last query block (QB = 16 QF NW rows) is ragged
        assert any(byid[c]["Nq"] % (16 * byid[c]["qf"] * byid[c]["nw"]) for c in what), f"{key}: reached only at whole query blocks"
        # every masked row: by a random mask and by a case with a wholly dead 64-key tile
        if key.split(", ")[5] == "true":
            assert any(byid[c]["mask"] == "rand" for c in what), f"{key}: no random mask"
            assert any(byid[c]["mask"] in ("lead", "trail", "all") for c in what), f"{key}: no case with a wholly dead key tile"
        # every rel-pos row: by a grid with kH != kW
        if key.split(", ")[4] != "0":
            assert any(byid[c]["rel"][0] != byid[c]["rel"][1] for c in what), f"{key}: no grid with kH != kW"
    listed = {c for row in RC.ATTN_GENERAL_LEDGER.values() for c in row[-1]}
    assert not ids - listed, f"cases that assert no route: {sorted(ids - listed)}"
    for c in RC.ATTN_GENERAL_CASES:
        assert c["op"] == "attn" and c["lay"] in ("qkv", "bhnd") and c.get("mask") in (None, "rand", "lead", "trail", "tailkey", "all"), c
        assert c["B"] == 2 and c["B"] * c["H"] <= 6 and (c["Nq"] * c["Nk"] <= 512 * 512 or c["qf"] == 4), c
        assert not c.get("rel") or c["rel"][0] * c["rel"][1] == c["Nk"], c
        assert c.get("mask") != "tailkey" or c["Nk"] % 64, c
        assert c.get("mask") not in ("lead", "trail") or c["Nk"] > 64, c


def test_ledger_equals_the_compiled_instantiations(tmp_path):
    keys = compiled_instantiations(tmp_path)
    assert len(keys) == len(set(keys)), "a kernel key appears twice"
    ledger = set(RC.LEDGER) | set(RC.NORM_LEDGER) | set(RC.ROWPANEL_LEDGER) | set(RC.ATTN_GENERAL_LEDGER)
    # (equality with the ledger's own count per family: a regular expression that silently finds nothing cannot pass)
    for family in ("gemm_kernel<", "attn_fast_kernel<", "attn_pipe_kernel<", "attn_kernel<") + tuple(f + "<" for f in NORM_FAMILIES + ROWPANEL_FAMILIES) + NORM_PLAIN:
        assert sum(k.startswith(family) for k in keys) == sum(k.startswith(family) for k in ledger) > 0, (family, keys)
    compiled = set(keys)
    assert not compiled - ledger, f"instantiations without a ledger row (classify them in tests/route_cases.py): {sorted(compiled - ledger)}"
    assert not ledger - compiled, f"ledger rows for instantiations the default build no longer compiles: {sorted(ledger - compiled)}"


@pytest.mark.gpu
def test_route_cases_on_gpu():
    env = {k: v for k, v in os.environ.items() if not k.startswith("AE_")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "route_check.py")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=1200)
    print(p.stdout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ROUTE_SUMMARY ")]
    assert lines, f"route_check.py ended without a summary (exit {p.returncode}):\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
    summary = json.loads(lines[-1][len("ROUTE_SUMMARY "):])
    assert summary["aborted"] is None, f"GPU work stopped at {summary['aborted']}"
    results = {r["id"]: r for r in summary["results"]}
    assert set(results) == set(RC.CASE_IDS), sorted(set(RC.CASE_IDS) - set(results))
    failed = {i: r["error"] for i, r in results.items() if not r["ok"]}
    assert not failed, failed
    unreached = [(k, c) for k, (kind, cases) in RC.LEDGER.items() if kind == "default" for c in cases if k not in results[c]["keys"]]
    assert not unreached, unreached
    attn = [c["id"] for c in RC.CASES if c["op"] == "attn"]
    no_lse = [i for i in attn if not isinstance(results[i].get("lse_ratio"), float) or not results[i]["lse_ratio"] <= 1.0]
    assert not no_lse, f"attention cases without a checked log-sum-exp: {no_lse}"
    print("lse_ratio per attention case: " + ", ".join(f"{i} {results[i]['lse_ratio']:.3f}" for i in attn))
    assert p.returncode == 0, p.stderr[-4000:]


@pytest.mark.gpu
def test_norm_route_cases_on_gpu():
    """norm.hip: every case reaches its rows, passes the statistics and element-wise float64 checks (tests/norm_ref.py), leaves its guards
    untouched and repeats bit for bit; prints the worst error / bound per case and the conditioning sweep (reported, not asserted)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("AE_")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "norm_route_check.py")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=NORM_CHILD_TIMEOUT)
    print(p.stdout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("NORM_ROUTE_SUMMARY ")]
    assert lines, f"norm_route_check.py ended without a summary (exit {p.returncode}):\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
    summary = json.loads(lines[-1][len("NORM_ROUTE_SUMMARY "):])
    assert summary["aborted"] is None, f"GPU work stopped at {summary['aborted']}"
    results = {r["id"]: r for r in summary["results"]}
    assert set(results) == set(RC.NORM_CASE_IDS), sorted(set(RC.NORM_CASE_IDS) - set(results))
    failed = {i: r["error"] for i, r in results.items() if not r["ok"]}
    assert not failed, failed
    unreached = [(k, c) for k, (kind, cases) in RC.NORM_LEDGER.items() for c in cases if k not in results[c]["keys"]]
    assert not unreached, unreached
    assert all(r["guards"] == "intact" and isinstance(r["ratio"], float) and r["ratio"] <= 1.0 for r in results.values())
    no_stat = [c["id"] for c in RC.NORM_CASES if (c["op"] == "gnb" and c["saved"] or c["op"] == "gn" and c["stat"])
               and not (isinstance(results[c["id"]]["stat_ratio"], float) and results[c["id"]]["stat_ratio"] <= 1.0)]
    assert not no_stat, f"GroupNorm cases without checked statistics: {no_stat}"
    print("worst error / bound per case (output, statistics): " + ", ".join(
        f"{i} {r['ratio']:.3f}" + (f" {r['stat_ratio']:.3f}" if r["stat_ratio"] is not None else "") for i, r in results.items()))
    print("conditioning sweep, worst |rstd^/rstd - 1| per route and |mean|/sigma: " + json.dumps(summary["conditioning"]))
    assert p.returncode == 0, p.stderr[-4000:]


def _rowpanel_child(env_name):
    env = {k: v for k, v in os.environ.items() if not k.startswith("AE_")}
    if env_name == "hook":
        env["AE_ROWPANEL_ANY_M"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rowpanel_route_check.py"), "--env", env_name], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=ROWPANEL_CHILD_TIMEOUT)
    print(p.stdout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ROWPANEL_ROUTE_SUMMARY ")]
    assert lines, f"rowpanel_route_check.py --env {env_name} ended without a summary (exit {p.returncode}):\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
    summary = json.loads(lines[-1][len("ROWPANEL_ROUTE_SUMMARY "):])
    assert summary["aborted"] is None, f"GPU work stopped at {summary['aborted']}"
    assert p.returncode in (0, 1), p.stderr[-4000:]
    return summary["results"]


@pytest.mark.gpu
def test_rowpanel_route_cases_on_gpu():
    """gemm_rowpanel.hip / ff_fused.hip: every case reaches its ledger rows (the two cases below the plan threshold: the tiled gemm_kernel), passes
    the element-wise float64 checks of tests/rowpanel_ref.py on every row, leaves its guards untouched and repeats bit for bit; prints the worst
    error / bound per case and per instantiation."""
    results = {r["id"]: r for env_name in ("hook", "default") for r in _rowpanel_child(env_name)}
    assert set(results) == set(RC.ROWPANEL_CASE_IDS), sorted(set(RC.ROWPANEL_CASE_IDS) ^ set(results))
    failed = {i: r["error"] for i, r in results.items() if not r["ok"]}
    assert not failed, failed
    unreached = [(k, c) for k, (kind, cases) in RC.ROWPANEL_LEDGER.items() for c in cases if k not in results[c]["keys"]]
    assert not unreached, unreached
    for c in RC.ROWPANEL_CASES:
        if c.get("tiled"):
            keys = results[c["id"]]["keys"]
            assert any(k.startswith("gemm_kernel<") for k in keys) and not any(k.startswith(ROWPANEL_FAMILIES) for k in keys), (c["id"], keys)
    assert all(r["guards"] == "intact" and isinstance(r["ratio"], float) and r["ratio"] <= 1.0 and all(v <= 1.0 for v in r["parts"].values())
               for r in results.values())
    print("worst error / bound per case: " + ", ".join(f"{i} {r['ratio']:.3f}" for i, r in results.items()))
    print("worst error / bound per instantiation: " + ", ".join(
        f"{k} {max(results[c]['ratio'] for c in cases):.3f}" for k, (kind, cases) in RC.ROWPANEL_LEDGER.items()))


def _attn_general_child(env_name):
    env = {k: v for k, v in os.environ.items() if not k.startswith("AE_")}
    env.update(RC.ATTN_GENERAL_ENVS[env_name])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "attn_general_route_check.py"), "--env", env_name], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=ATTN_GENERAL_CHILD_TIMEOUT)
    print(p.stdout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ATTN_GENERAL_SUMMARY ")]
    assert lines, f"attn_general_route_check.py --env {env_name} ended without a summary (exit {p.returncode}):\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
    summary = json.loads(lines[-1][len("ATTN_GENERAL_SUMMARY "):])
    assert summary["aborted"] is None, f"GPU work stopped at {summary['aborted']}"
    assert p.returncode in (0, 1), p.stderr[-4000:]
    return summary["results"]


@pytest.mark.gpu
def test_attn_general_route_cases_on_gpu():
    """attention.hip: every case reaches its ledger rows in its row's environment, leaves its guards and pad columns untouched, repeats bit for
    bit, leaves no sentinel in out / lse / lse2 and passes the element-wise float64 checks on every row of every (batch, head); prints the worst
    error / bound (output, log-sum-exp) per instantiation.  One child per environment, one after another: a child that faults, aborts or runs out
    of time fails the test there (no summary line, a non-zero exit, or subprocess.TimeoutExpired) and the remaining children are not started."""
    results = {}
    for env_name in RC.ATTN_GENERAL_ENVS:
        results.update({r["id"]: r for r in _attn_general_child(env_name)})
    assert set(results) == set(RC.ATTN_GENERAL_CASE_IDS), sorted(set(RC.ATTN_GENERAL_CASE_IDS) ^ set(results))
    failed = {i: r["error"] for i, r in results.items() if not r["ok"]}
    assert not failed, failed
    unreached = [(k, c) for k, row in RC.ATTN_GENERAL_LEDGER.items() for c in row[-1] if k not in results[c]["keys"]]
    assert not unreached, unreached
    assert all(r["guards"] == "intact" and isinstance(r["ratio"], float) and r["ratio"] <= 1.0 and isinstance(r["lse_ratio"], float)
               and r["lse_ratio"] <= 1.0 for r in results.values())
    print("worst error / bound per instantiation (output, log-sum-exp): " + ", ".join(
        f"{k} {max(results[c]['ratio'] for c in row[-1]):.3f} {max(results[c]['lse_ratio'] for c in row[-1]):.3f}"
        for k, row in RC.ATTN_GENERAL_LEDGER.items()))
