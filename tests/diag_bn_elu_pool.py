"""Diagnostic (not a test): measures expm1f and __expf alone against float64, runs tests/test_gpu_bn_elu_pool.py on the GPU and
assembles profiles/bn_elu_pool_edges.json from the record the tests write: per row the plan's route and the worst error / tolerance
per output; per table and regime the worst ratio and where; for the offset rows the error in units of sigma against |mean| / sigma;
which rows stand for every plan class, regime and seeded defect; the model row's figures; the wall time of the GPU file.

The intrinsics are measured through two entry points that reduce to them: ign_affine_elu_pool_fwd at P = 1, scale 1, shift 0 is
expm1f(v) for v <= 0 (the fma is exact); ign_bn_elu_pool_bwd_apply at P = 1, ka = 1, kb = kc = 0, dout = 1 is __expf(v).  The
constants C_EXPM1 / C_EXPF of tests/bn_elu_pool_cases.py are twice the maxima recorded here.

Usage: python tests/diag_bn_elu_pool.py --out profiles/bn_elu_pool_edges.json"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import bn_elu_pool_cases as K  # noqa: E402


def _sig(x, n=4):
    if isinstance(x, float) and (x != x or abs(x) == float("inf")):
        return str(x)
    return float(f"{x:.{n}g}") if isinstance(x, float) else x


def _ulp_of(ref):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126))) - 23)


def measure_intrinsics():
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    L, dev = _lib.lib(), torch.device("cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rng = np.random.default_rng(0)
    z = np.concatenate([-np.logspace(-30, 2, 200001), -rng.uniform(0, 1, 400000), -rng.uniform(0, 20, 400000),
                        -rng.uniform(20, 87, 200000), -rng.uniform(87, 110, 50000), -(2.0 ** -np.arange(0, 40)), [-0.0, 0.0]]).astype(np.float32)
    T = 1024
    z = np.concatenate([z, np.full((-z.size) % T, -1.0, np.float32)])
    B = z.size // T
    v = torch.from_numpy(z.reshape(B, 1, T)).to(dev)
    one, zero = torch.ones(1, device=dev), torch.zeros(1, device=dev)
    out, dv, dout = torch.empty(B, 1, T, device=dev), torch.empty(B, 1, T, device=dev), torch.ones(B, 1, T, device=dev)
    _lib.check(L.ign_affine_elu_pool_fwd(p(v), p(one), p(zero), p(out), B, 1, T, 1, _lib.stream()), "ign_affine_elu_pool_fwd")
    _lib.check(L.ign_bn_elu_pool_bwd_apply(p(v), p(dout), p(one), p(zero), p(one), p(zero), p(zero), p(dv), B, 1, T, 1, _lib.stream()),
               "ign_bn_elu_pool_bwd_apply")
    torch.cuda.synchronize()
    em1, ex, z64 = out.cpu().numpy().reshape(-1).astype(np.float64), dv.cpu().numpy().reshape(-1).astype(np.float64), z.astype(np.float64)
    res = dict(points=int(z.size), range="z in [-110, 0]")
    ref = np.expm1(z64)
    e = np.abs(em1 - ref) / _ulp_of(ref)
    res["expm1f"] = dict(max_ulp=_sig(float(e.max())), at_z=_sig(float(z64[int(np.argmax(e))])), constant=K.C_EXPM1)
    normal = z64 >= -87
    hw = np.exp2((z * np.float32(K.LOG2E)).astype(np.float32).astype(np.float64))
    e = (np.abs(ex - hw) / _ulp_of(hw))[normal]
    res["expf_vs_exp2_of_fp32_product"] = dict(max_ulp=_sig(float(e.max())), at_z=_sig(float(z64[normal][int(np.argmax(e))])),
                                               constant=K.C_EXPF)
    ref = np.exp(z64)
    rel = (np.abs(ex - ref) / ref / K.ULP)[normal]
    res["expf_vs_exp"] = dict(max_rel_error_in_ulp=_sig(float(rel.max())),
                              worst_of_model=_sig(float((rel / (np.abs(z64[normal]) * K.LOG2E + K.C_EXPF)).max())),
                              model="(|z| log2 e + C_EXPF) 2^-23 relative")
    res["expf_below_-87"] = {"max_abs_error_over_2^-126": _sig(float(np.abs(ex[~normal] - ref[~normal]).max() / K.TINY))}
    res["at_zero"] = dict(expf=float(ex[z64 == 0].min()), expm1f=float(np.abs(em1[z64 == 0]).max()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import pytest
    intr = measure_intrinsics()
    print("intrinsics", json.dumps(intr))
    with tempfile.TemporaryDirectory() as tmp:
        rec_path = os.path.join(tmp, "record.json")
        os.environ["IGN_BN_ELU_POOL_OUT"] = rec_path
        t0 = time.perf_counter()
        rc = int(pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "--durations=8", "--maxfail=5", os.path.join(HERE, "test_gpu_bn_elu_pool.py")]))
        wall = time.perf_counter() - t0
        record = json.load(open(rec_path)) if os.path.exists(rec_path) else {}
    refusals = record.pop("refusals", {})
    worst, per_row, n_cmp, n_failed, dc = {}, {}, 0, 0, []
    for table, rows in sorted(record.items()):
        for name, rec in sorted(rows.items()):
            regime = name.rsplit("-", 1)[-1] if table in ("direct", "op_train", "op_eval") else table
            outs = {}
            for what, r in rec["outputs"].items():
                n_cmp += 1
                n_failed += not r["ratio"] <= 1.0
                outs[what] = _sig(float(r["ratio"]))
                slot = worst.setdefault(table, {}).setdefault(regime, {})
                key = what.split(":")[-1] if "repeats" not in what else "repeats"
                if key not in slot or r["ratio"] > slot[key]["ratio"]:
                    slot[key] = dict(ratio=_sig(float(r["ratio"])), row=name)
            row = dict(route=rec["route"], worst_ratio_per_output={k: v for k, v in outs.items() if "repeats" not in k},
                       repeats_bitwise=all(v == 0.0 for k, v in outs.items() if "repeats" in k))
            for k in ("dalpha_over_dgamma", "dalpha_tol_over_dalpha"):
                if rec.get(k) is not None:
                    row[k] = _sig(rec[k])
            if "dc_sensitivity" in rec:
                row["dc_sensitivity"] = {k: _sig(v) for k, v in rec["dc_sensitivity"].items()}
                dc.append(dict(row=name, **row["dc_sensitivity"]))
            if table == "model":
                row["outputs"] = {k: {a: _sig(b) for a, b in v.items()} for k, v in rec["outputs"].items()}
            per_row.setdefault(table, {})[name] = row
    cs = K.cases()
    classes = {cl: sorted(c.id for c in cs if cl in K.plan(c)["classes"]) for cl in sorted(K.all_classes())}
    out = dict(
        what="tests/test_gpu_bn_elu_pool.py on one MI355X: ops.bn_elu_pool and the six entry points behind it against float64",
        metric="per element |got - float64| / tolerance (tests/bn_elu_pool_cases.py: d u sum|terms| for sums, interval propagation + 2 "
               "ulp for the fold outputs, K u of the terms per element for out and dv, dalpha at the bound of its own S2 with no floor); "
               "0 ('exact') = must be equal",
        pytest_exit_code=rc, comparisons=n_cmp, comparisons_outside_their_tolerance=n_failed, wall_seconds_of_the_gpu_file=round(wall, 1),
        intrinsics=intr,
        table=dict(rows=len(cs), per_regime={r: sum(c.regime == r for c in cs) for r in K.OP_REGIMES + K.DIRECT_REGIMES},
                   refusals=refusals, host_branches=[b[0] for b in K.HOST_BRANCHES]),
        plan_classes={cl: dict(rows=len(ids), first=ids[0] if ids else None) for cl, ids in classes.items()},
        seeded_defects=dict({d: dict(breaks=cl, rows_of_that_class=len(classes[cl])) for d, cl in K.DEFECTS.items()},
                            **{K.CONTROL_DEFECT: dict(control=True, flagged_in_gauss_rows=False)}),
        dc_sensitivity=dc,
        worst_ratio=worst,
        per_row=per_row,
    )
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}: {n_failed} of {n_cmp} comparisons outside their tolerance, {wall:.1f} s")
    return rc


if __name__ == "__main__":
    sys.exit(main())
