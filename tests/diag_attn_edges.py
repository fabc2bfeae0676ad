"""Diagnostic (not a test): runs tests/test_gpu_attn_edges.py on the GPU and assembles profiles/attn_edges.json from the record the
tests write: per case and tensor the kernel's error, the tolerance it was held to and their ratio (regime cases: also the error of
the float32 restatement the tolerance is derived from), the worst ratio per (arithmetic, head width) route and per section, what
the host side says the table covers, and the wall time of the GPU file.

Usage: python tests/diag_attn_edges.py --out profiles/attn_edges.json [--bench FILE]
--bench FILE: a JSON object to store under "bench" (step times of bench.py's transformer configuration, parent and this tree
alternating; only needed when a kernel changed)."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import attn_edge_cases as C  # noqa: E402


def _sig(x, n=4):
    if isinstance(x, float) and (x != x or abs(x) == float("inf")):
        return str(x)                                                   # "inf" / "nan": strict JSON has no such numbers
    return float(f"{x:.{n}g}") if isinstance(x, float) else x


def _route_of(section, name):
    """"<arith> E=<E> ..." / "<regime> <arith> E=<E>" -> "arith E=.."; the unrouted and view cases have routes of their own"""
    if section == "unrouted":
        return "bf16x6 backward E=128 (C ABI only)"
    if section == "views":
        return "default arithmetic E=32"
    m = re.search(r"(f32|bf16x6|f16x3|bf16) E=(\d+)", name)
    return f"{m.group(1)} E={m.group(2)}"


def _bf16_tolerances():
    from test_gpu_bf16_parity import ATTN_TOL, ATTN_TOL_RMS
    out = {}
    for r in C.REGIMES:
        for E in C.REGIME_WIDTHS:
            if ("bf16", E) in C.ROUTES:
                out[f"{r} E={E}"] = {w: dict(tol=[_sig(t[0]), _sig(t[1])], noise=[_sig(n[0]), _sig(n[1])],
                                             tol_over_parity_bound=[_sig(t[0] / ATTN_TOL), _sig(t[1] / ATTN_TOL_RMS)])
                                     for w, (t, n) in C.bf16_regime_tolerances(r, E).items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--bench")
    args = ap.parse_args()
    import pytest
    with tempfile.TemporaryDirectory() as tmp:
        rec_path = os.path.join(tmp, "record.json")
        os.environ["IGN_ATTN_EDGES_OUT"] = rec_path
        t0 = time.perf_counter()
        rc = int(pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "--durations=5", os.path.join(HERE, "test_gpu_attn_edges.py")]))
        wall = time.perf_counter() - t0
        record = json.load(open(rec_path)) if os.path.exists(rec_path) else {}
    worst_route, worst_section, n_cases, n_failed = {}, {}, 0, 0
    for section, cases in record.items():
        for name, tensors in cases.items():
            n_cases += 1
            route = _route_of(section, name)
            for what, r in tensors.items():
                n_failed += not r["err"] <= r["tol"]
                for table, key in ((worst_route, route), (worst_section, section)):
                    if key not in table or r["ratio"] > table[key]["raw"]:
                        table[key] = dict(raw=r["ratio"], ratio=_sig(r["ratio"]), case=f"{section} {name}", tensor=what, err=_sig(r["err"]), tol=_sig(r["tol"]))
    worst = max(worst_route.values(), key=lambda r: r["raw"], default=None)
    for table in (worst_route, worst_section):
        for r in table.values():
            r.pop("raw")
    out = dict(
        what="tests/test_gpu_attn_edges.py on one MI355X: error / tolerance per case and tensor (tests/attn_edge_cases.py)",
        metric="fp32-accurate routes: max over (batch, head) slices of max|got - ref| / max|ref| against float64; bf16 route: "
               "whole-tensor max and rms against the rounded-operand float64 model of tests/test_gpu_bf16_parity.py",
        bounds=dict(forward=C.FWD_TOL, gradients=C.GRAD_TOL, map_row_sums=C.MAP_ROWSUM_TOL, regime_margin=C.REGIME_MARGIN,
                    regime_max_factor=C.REGIME_MAX_FACTOR),
        pytest_exit_code=rc, cases=n_cases, comparisons_outside_their_tolerance=n_failed, wall_seconds_of_the_gpu_file=round(wall, 1),
        worst_ratio=worst, worst_ratio_per_route=dict(sorted(worst_route.items())), worst_ratio_per_section=worst_section,
        regime_fp32_restatement={f"{r} E={E}": {w: dict(fp32_err=_sig(e), tol=_sig(t)) for w, (t, e, _) in C.regime_tolerances(r, E).items()}
                                 for r in C.REGIMES for E in C.REGIME_WIDTHS},
        # the bf16 route's regime rows: tolerance and the model's own noise it is derived from, each as (max, rms), and both as
        # multiples of the bounds of tests/test_gpu_bf16_parity.py (never above regime_max_factor: tests/test_attn_edges_host.py)
        regime_bf16_tolerances=_bf16_tolerances(),
        bf16_rows_rescaled=C.BF16_RESCALED,
        edge_pairs=C.EDGE_PAIRS, routes=[f"{a} E={E}" for a, E in C.ROUTES],
        # [error, tolerance, ratio(, error of the float32 restatement)]
        records={s: {n: {w: [_sig(r["err"]), _sig(r["tol"]), _sig(r["ratio"])] + ([_sig(r["fp32_restatement"])] if "fp32_restatement" in r else [])
                         for w, r in t.items()} for n, t in cs.items()} for s, cs in record.items()},
    )
    if args.bench:
        out["bench"] = json.load(open(args.bench))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("{\n")
        keys = list(out)
        for i, k in enumerate(keys):
            end = ",\n" if i + 1 < len(keys) else "\n"
            if k == "records":
                f.write(' "records": {\n')
                secs = list(out[k])
                for j, s in enumerate(secs):
                    f.write(f'  {json.dumps(s)}: {{\n')
                    names = sorted(out[k][s])
                    f.write(",\n".join(f"   {json.dumps(n)}: {json.dumps(out[k][s][n])}" for n in names))
                    f.write("\n  }" + (",\n" if j + 1 < len(secs) else "\n"))
                f.write(" }" + end)
            else:
                f.write(f" {json.dumps(k)}: {json.dumps(out[k])}{end}")
        f.write("}\n")
    print(f"wrote {args.out}: {n_cases} cases, {n_failed} comparisons outside their tolerance, worst ratio {worst}, {wall:.1f} s")
    return rc


if __name__ == "__main__":
    sys.exit(main())
