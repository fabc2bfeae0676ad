"""Diagnostic (not a test): runs tests/test_gpu_glue_edges.py on the GPU and assembles profiles/glue_edges.json from the record the
tests write: per case the route, the chain length d and the worst error / tolerance; per entry point the worst ratio (with the case
and output it occurred at) in the Gaussian and in the exact regime; what the table holds; and the wall time of the GPU file.

Usage: python tests/diag_glue_edges.py --out profiles/glue_edges.json"""
import argparse
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import glue_edge_cases as G  # noqa: E402


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
        os.environ["IGN_GLUE_EDGES_OUT"] = rec_path
        t0 = time.perf_counter()
        rc = int(pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "--durations=8", os.path.join(HERE, "test_gpu_glue_edges.py")]))
        wall = time.perf_counter() - t0
        record = json.load(open(rec_path)) if os.path.exists(rec_path) else {}
    worst, per_case, n_cmp, n_failed = {}, {}, 0, 0
    for entry, cases in sorted(record.items()):
        for name, rec in sorted(cases.items()):
            regime = "exact" if name.rsplit(" ", 1)[-1] in ("exact", "negative") else "bounded"
            top, top_out, d = 0.0, None, 0
            for what, r in rec["outputs"].items():
                n_cmp += 1
                n_failed += not r["ratio"] <= 1.0
                d = max(d, r.get("d", 0))
                if r["ratio"] >= top:
                    top, top_out = r["ratio"], what
            per_case.setdefault(entry, {})[name] = dict(route=rec["route"], d=d, worst_ratio=_sig(top), at=top_out)
            slot = worst.setdefault(entry, {})
            if regime not in slot or top > slot[regime]["ratio"]:
                slot[regime] = dict(ratio=_sig(top), case=name, output=top_out, d=d)
    out = dict(
        what="tests/test_gpu_glue_edges.py on one MI355X: worst error / tolerance per entry point of csrc/ign_head.hip and csrc/ign_bn.hip",
        metric="per element |got - float64| / tolerance; tolerance = d * 2^-24 * sum|a||b| + 1 ulp for sums (d = serial fp32 additions, "
               "at most 96), a stated number of ulps for elementwise outputs, interval propagation + 2 ulp for the finalize outputs, "
               "1e-5 relative / 1e-4 of the maximum for the diversity and regulariser loss / gradient; 0 ('exact') = must be equal",
        pytest_exit_code=rc, cases=sum(len(v) for v in record.values()), comparisons=n_cmp, comparisons_outside_their_tolerance=n_failed,
        wall_seconds_of_the_gpu_file=round(wall, 1),
        table=dict(cases=len(G.cases()), per_entry={e: len(G.of(e)) for e in sorted({c.entry for c in G.cases()})}, refusals=len(G.REFUSALS),
                   workspace_sequences=2),
        worst_ratio_per_entry_point=worst,
        per_case=per_case,
    )
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}: {out['cases']} cases, {n_failed} of {n_cmp} comparisons outside their tolerance, {wall:.1f} s")
    for e, w in sorted(worst.items()):
        print(" ", e, w)
    return rc


if __name__ == "__main__":
    sys.exit(main())
