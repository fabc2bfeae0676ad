"""Diagnostic (not a test): assembles profiles/shapelet_bwd_plan.json, the record of the shapelet weight-backward launch-plan
tests.  Per row of tests/shapelet_bwd_plan_cases.py: the plan fields and the reducers its nbs selects (the Python restatement of
tests/test_shapelet_bwd_plan_host.py; with the library built, ign_shapelet_bwd_plan is asked as well and must agree); per planted
defect of the host module, the error of the fault-free float32 restatement and of the restatement with the defect, both as
multiples of the 1e-4 tolerance of the GPU comparison.  Needs no GPU.

--gpu-record FILE: the JSON that tests/test_gpu_shapelet_bwd_plan.py writes with IGN_SHAPELET_BWD_PLAN_OUT=FILE on an MI355X
  (observed errors as multiples of the tolerance, wall times); merged row by row.
Usage: python tests/diag_shapelet_bwd_plan.py [--gpu-record FILE] --out profiles/shapelet_bwd_plan.json"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import shapelet_bwd_plan_cases as T  # noqa: E402
import test_shapelet_bwd_plan_host as H  # noqa: E402

SHOW = ("JJ", "cpk", "kb", "nkt", "last_tile", "threads", "tc", "nch", "last_chunk", "xs_len", "lds", "njt", "nbs", "capped",
        "reducer", "bank", "per", "batches", "tails", "empty_slices")


def _library():
    try:
        import speech_imagery_eeg_amd  # noqa: F401
        from ign_hip import _lib
        return _lib.lib() if os.path.exists(_lib.lib_path()) else None
    except Exception:
        return None


def rows():
    L = _library()
    out = {}
    for case_id, shape, mode, branch, _ in T.CASES:
        d = H.describe(shape)
        row = dict(shape=list(shape), mode=mode, branch=branch)
        if d["refused"]:
            row["plan"] = dict(refused=True, rc=d["rc"])
        else:
            row["plan"] = {k: d[k] for k in SHOW}
            row["plan"]["rows_per_slice"] = sorted(d["rows_per_slice"])
            dist, tie, strided = T.instantiation(shape, mode)
            row["kernel"] = dict(distance=dist, tie_exact=tie, body="strided" if strided else f"JJ={d['JJ']}",
                                 gate="lts" if mode & T.LTS else "rbf")
        if L is not None:
            got = H.lib_plan(L, shape)
            want = d["rc"] if d["refused"] else {k: d[k] for k in H.PLAN_FIELDS}
            assert got == want, (case_id, got, want)
            row["agrees_with_ign_shapelet_bwd_plan"] = True
        out[case_id] = row
    return out


def teeth():
    out = {}
    for defect in H.DEFECTS:
        t0 = time.perf_counter()
        clean, planted, _, _, _ = H.teeth_margins(defect)
        out[defect] = dict(row=T.TEETH[defect], tolerance=T.GRAD_TOL, fault_free_restatement_over_tol=clean, planted_over_tol=planted,
                           required_over_tol=10.0, seconds=time.perf_counter() - t0)
        print(f"{defect} at {T.TEETH[defect]}: fault-free {clean:.4f} x tol, planted {planted:.1f} x tol", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu-record", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = dict(tolerances=dict(values_elementwise=T.VAL_TOL, gradients_of_own_scale=T.GRAD_TOL), rows=rows(), teeth=teeth())
    if a.gpu_record:
        with open(a.gpu_record) as f:
            rec = json.load(f)["gpu_rows"]
        worst = {}
        for case_id, r in rec.items():
            out["rows"][case_id]["mi355x"] = {k: r[k] for k in ("errors_over_tol", "routes_bitwise_equal", "oracle_on",
                                                                "reference_channels", "seconds")}
            for route, errs in r["errors_over_tol"].items():
                for name, e in errs.items():
                    if e > worst.get(name, (0.0,))[0]:
                        worst[name] = (e, case_id, route)
        out["worst_observed_over_tol"] = {k: dict(error_over_tol=v[0], row=v[1], route=v[2]) for k, v in worst.items()}
        out["slowest_row_seconds"] = max((r["seconds"]["total"], i) for i, r in rec.items())
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
    else:
        json.dump(out, sys.stdout, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
