"""Diagnostic (not a test): runs tests/test_gpu_conv_edges.py on the GPU and assembles profiles/conv_edges.json from the record the
tests write: the worst error / tolerance per kernel, arithmetic and regime (with the case and output it occurred at), the
reference-side terms of that case's tolerance, what the table holds, and the wall time of the GPU file.

Usage: python tests/diag_conv_edges.py --out profiles/conv_edges.json"""
import argparse
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import conv_edge_cases as C  # noqa: E402


def _sig(x, n=4):
    if isinstance(x, float) and (x != x or abs(x) == float("inf")):
        return str(x)
    return float(f"{x:.{n}g}") if isinstance(x, float) else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import pytest
    with tempfile.TemporaryDirectory() as tmp:
        rec_path = os.path.join(tmp, "record.json")
        os.environ["IGN_CONV_EDGES_OUT"] = rec_path
        t0 = time.perf_counter()
        rc = int(pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "--durations=8", os.path.join(HERE, "test_gpu_conv_edges.py")]))
        wall = time.perf_counter() - t0
        record = json.load(open(rec_path)) if os.path.exists(rec_path) else {}
    worst, n_cases, n_cmp, n_failed = {}, 0, 0, 0
    for kernel, ariths in record.items():
        for arith, regimes in ariths.items():
            for regime, cases in regimes.items():
                for name, outs in cases.items():
                    n_cases += 1
                    for what, r in outs.items():
                        n_cmp += 1
                        n_failed += not r["err"] <= r["tol"]
                        slot = worst.setdefault(kernel, {}).setdefault(arith, {})
                        if regime not in slot or r["ratio"] > slot[regime]["ratio"]:
                            slot[regime] = dict(ratio=r["ratio"], case=name, output=what, err_units=r["err"], tol_units=r["tol"],
                                                **{k: r[k] for k in ("e_model", "e_acc", "K") if k in r})
    top = max((r["ratio"] for a in worst.values() for g in a.values() for r in g.values()), default=None)
    out = dict(
        what="tests/test_gpu_conv_edges.py on one MI355X: worst error / tolerance per kernel, arithmetic and operand regime",
        metric="per element |got - float64| in units of 2^-24 * cond, cond = sum |a||b| (+ |bias|) over the element's reduction; the "
               "bf16 route against the float64 product of the bf16-rounded operands; 'partials s1 / s2': the statistics partials "
               "against float64 sums of the kernel's own outputs in units of (rows + 4) * 2^-24 * sum |term|",
        tolerance="E_model + max(1, 4 * E_acc) units, never above min(16, K + 8) (tests/conv_edge_cases.py)",
        pytest_exit_code=rc, cases=n_cases, comparisons=n_cmp, comparisons_outside_their_tolerance=n_failed,
        wall_seconds_of_the_gpu_file=round(wall, 1), worst_ratio=_sig(top) if top is not None else None,
        table=dict(cases=len(C.CASES), runs=len(C.runs()), refused=sum(len(C.refused_ariths(c)) for c in C.CASES),
                   draws_above_the_first={f"{c.kind} {c.name}": C.draw_of(c) for c in C.CASES if C.draw_of(c)}),
        worst_ratio_per_kernel_arithmetic_regime={k: {a: {g: {f: _sig(v) for f, v in r.items()} for g, r in sorted(gs.items())}
                                                      for a, gs in sorted(ar.items())} for k, ar in sorted(worst.items())},
    )
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}: {n_cases} cases, {n_failed} of {n_cmp} comparisons outside their tolerance, worst ratio {top}, {wall:.1f} s")
    return rc


if __name__ == "__main__":
    sys.exit(main())
