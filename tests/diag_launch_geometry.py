"""Diagnostic (not a test): what float32 arithmetic in the kernels' own summation order costs at the shapes of
tests/test_gpu_launch_geometry.py, what the planted defects of tests/test_launch_geometry_host.py cost, and the assembly of
profiles/launch_geometry.json.  Needs no GPU.

--layernorm: per LayerNorm shape with more than one row group per wave, d(gamma) and d(beta) of the float32 restatement
  (ln_stats_f32 + ln_param_grads_f32: per-lane accumulation over the row groups, the slots of a block in order, 16 slices of blocks,
  then the slices) against float64 numpy, relative to the gradient's maximum -- the figure the 1e-5 bounds of the GPU test are
  held against; and the integer-gy column sums with and without a skipped row group.  --no-cap leaves out the 4.2 M-row shape.
--instnorm: per instance-norm shape, xn of the float32 restatement (instnorm_fwd_f32) against float64, element-wise as the GPU
  test judges it, and the same with one sample missing from the statistics / the ragged last tile on stale statistics.
--cases FILE (repeatable): a JSON file merged into the output.  A parity ledger (the parity.json that tests/conftest.py writes when a `-m gpu` run ends) gives
  its entries for the tests of tests/test_gpu_launch_geometry.py under "gpu_parity"; any other object (the wall times written
  with IGN_LAUNCH_GEOMETRY_OUT) is merged key by key.
Usage: python tests/diag_launch_geometry.py --layernorm --instnorm [--cases parity.json] --out profiles/launch_geometry.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import test_launch_geometry_host as H  # noqa: E402


def _rel(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


def _elem(a, ref):
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(a, np.float64) - ref) / (1.0 + np.abs(ref))).max())


def layernorm(with_cap):
    rows = {}
    for (R, D) in H.LN_SHAPES:
        geo = H.ln_geometry(R, D)
        if geo["iters"] == 1 or ((R, D) == H.LN_CAP_SHAPE and not with_cap):
            continue
        t0 = time.perf_counter()
        rng = np.random.default_rng(R + D)
        x = (rng.standard_normal((R, D), dtype=np.float32) * np.float32(3) + np.float32(1.5))
        gy = rng.standard_normal((R, D), dtype=np.float32)
        mean, rstd = H.ln_stats_f32(x, geo)
        dg, db = H.ln_param_grads_f32(x, gy, mean, rstd, geo)
        xd = x.astype(np.float64)
        m64 = xd.mean(-1, keepdims=True)
        xd -= m64
        r64 = 1.0 / np.sqrt((xd * xd).mean(-1, keepdims=True) + 1e-5)
        xd *= r64
        stats = dict(mean=_rel(mean, m64[:, 0]), rstd=_rel(rstd, r64[:, 0]))
        xd *= gy
        dg64, db64 = xd.sum(0), gy.astype(np.float64).sum(0)
        del xd
        gi = rng.integers(-2, 3, size=(R, D)).astype(np.float32)
        exact = gi.astype(np.int64).sum(0)
        zero, one = np.zeros(R, np.float32), np.ones(R, np.float32)
        _, dbi = H.ln_param_grads_f32(gi, gi, zero, one, geo)
        _, dbs = H.ln_param_grads_f32(gi, gi, zero, one, geo, defect="skip last group")
        row = dict(geometry={k: geo[k] for k in ("G", "nv", "rpw", "iters", "nblk", "per", "last")},
                   restated_fp32_vs_float64=dict(dgamma=_rel(dg, dg64), dbeta=_rel(db, db64), **stats),
                   bound_in_the_test=dict(dgamma=H.LN_TOL["dgamma"], dbeta=H.LN_TOL["dbeta"]),
                   integer_gy=dict(columns_off=int(np.count_nonzero(dbi != exact)),
                                   columns_off_with_one_row_group_skipped=int(np.count_nonzero(dbs != exact)),
                                   rows_skipped=geo["rpw"], relative_to_max=_rel(dbs, exact)),
                   seconds=time.perf_counter() - t0)
        rows[f"{R}x{D}"] = row
        print(f"LayerNorm {R}x{D} iters={geo['iters']} rpw={geo['rpw']}: restated fp32 vs float64 dgamma "
              f"{row['restated_fp32_vs_float64']['dgamma']:.2e} dbeta {row['restated_fp32_vs_float64']['dbeta']:.2e} | integer gy: "
              f"{row['integer_gy']['columns_off']} columns off, {row['integer_gy']['columns_off_with_one_row_group_skipped']} of {D} with "
              f"{geo['rpw']} rows skipped ({row['integer_gy']['relative_to_max']:.2e} of the maximum)  [{row['seconds']:.1f} s]", flush=True)
    return rows


def instnorm():
    rows = {}
    for (B, T, C) in H.INSTNORM_SHAPES:
        tile = H.instnorm_tile(T, C)
        x = H.instnorm_input(B, T, C)
        ref = H.instnorm_f64(x)
        row = dict(tile=tile, bound_in_the_test=H.XN_TOL, restated_fp32_vs_float64=_elem(H.instnorm_fwd_f32(x, tile["CT"]), ref),
                   one_sample_short=_elem(H.instnorm_fwd_f32(x, tile["CT"], defect="one sample short"), ref))
        if tile["CT"] > 1 and tile["tiles"][-1] < tile["CT"]:
            row["stale_tile_statistics"] = _elem(H.instnorm_fwd_f32(x, tile["CT"], defect="stale tile statistics"), ref)
        rows["B{} T{} C{}".format(B, T, C)] = row
        print(f"instance norm B={B} T={T} C={C} CT={tile['CT']} tiles={tile['tiles']}: restated fp32 vs float64 "
              f"{row['restated_fp32_vs_float64']:.2e} | one sample short {row['one_sample_short']:.2e} | stale tile statistics "
              f"{row.get('stale_tile_statistics', float('nan')):.2e}", flush=True)
    return rows


def _gpu_tests():
    """names of the test functions of the GPU module, read from its text (no torch, no import of the module)"""
    import re
    src = open(os.path.join(HERE, "test_gpu_launch_geometry.py")).read()
    return set(re.findall(r"^def (test_\w+)\(", src, flags=re.M))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layernorm", action="store_true")
    ap.add_argument("--no-cap", action="store_true")
    ap.add_argument("--instnorm", action="store_true")
    ap.add_argument("--cases", action="append", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {}
    if a.layernorm:
        out["layernorm_param_grads"] = layernorm(not a.no_cap)
    if a.instnorm:
        out["instnorm_forward"] = instnorm()
    for path in a.cases:
        with open(path) as f:
            rec = json.load(f)
        if "tests" in rec and "north_star_tol" in rec:
            names = _gpu_tests()
            out.setdefault("gpu_parity", {}).update({t: r for t, r in rec["tests"].items() if t.split("[")[0] in names})
        else:
            out.update(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
