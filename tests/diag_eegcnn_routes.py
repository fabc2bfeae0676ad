"""Diagnostic (not a test): assembles profiles/eegcnn_routes.json, the record of the EEG-CNN route tests.  Per row of
tests/eegcnn_route_cases.py: the route the row is there for, from the Python restatement of the dispatch rules (with the library
built, the block counts it can give without a device are asked as well and must agree); with --gpu-record, the error against
float64 that tests/test_gpu_eegcnn_routes.py observed on an MI355X and the bound it was held to.  Needs no GPU.

--gpu-record FILE: the JSON that tests/test_gpu_eegcnn_routes.py writes with IGN_EEGCNN_ROUTES_OUT=FILE.
Usage: python tests/diag_eegcnn_routes.py [--gpu-record FILE] --out profiles/eegcnn_routes.json"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import eegcnn_route_cases as R  # noqa: E402


def _library():
    try:
        import speech_imagery_eeg_amd  # noqa: F401
        from ign_hip import _lib
        return _lib.lib() if os.path.exists(_lib.lib_path()) else None
    except Exception:
        return None


def _plain(d):
    return {k: (sorted(v) if isinstance(v, set) else v) for k, v in d.items()}


def rows():
    L = _library()
    out = {}
    t = out["dwconv1d"] = {}
    for (B, C, T, k), want, why in R.DWCONV_CASES:
        t[str((B, C, T, k))] = dict(why=why, there_for=_plain(want), route=_plain(R.dwconv_route(T, k, B)))
    t = out["autocorr"] = {}
    for (Rr, T, K), want, why in R.AUTOCORR_CASES:
        t[str((Rr, T, K))] = dict(why=why, route=R.autocorr_route(T, K, Rr))
    t = out["window_gram"] = {}
    for (Rr, T, k, pl), want, why in R.GRAM_CASES:
        t[str((Rr, T, k, pl))] = dict(why=why, route=dict(lag_sums=R.autocorr_route(T, k, Rr)["kernel"], edges=R.gram_edges(k)))
    t = out["conv1_sumsq"] = {}
    for (Rr, T, F1, k1), why in R.SUMSQ_CASES:
        t[str((Rr, T, F1, k1))] = dict(why=why, route=dict(model_route=R.bn1_route(T, k1, F1, variance_switch="conv"),
                                                          longest_trainable_kernel=R.conv1_sumsq_max_taps(F1)))
    t = out["chan_contract"] = {}
    for (B, Ci, Co, T), off, want, why in R.CHAN_CASES:
        plan = R.cw_plan(B, T, aligned=off % 4 == 0)
        if L is not None:
            assert L.ign_chan_contract_bwd_weight_workspace_bytes(B, Ci, Co, T) == plan["blocks"] * Co * Ci * 4
            plan["blocks_agree_with_the_library"] = True
        t[f"{(B, Ci, Co, T)}+{off}"] = dict(why=why, base_offset_floats=off, route=plan)
    t = out["model"] = {}
    for name, shape, opts, route, why in R.MODEL_CASES:
        ks = R.model_kernels(shape, opts)
        assert ks["bn1"] == route, name
        t[name] = dict(why=why, shape=list(shape), options={k: repr(v) for k, v in opts.items()}, bn1_route=route,
                       lag_sums=ks.get("lag_sums"), block1={k: ks["block1"][k] for k in ("fwd", "TT", "dw")},
                       block2={k: ks["block2"][k] for k in ("fwd", "TT", "dw")})
    out["refusals"] = {
        "k1 beyond 128 taps": dict(shape=list(R.REFUSED_TAPS["shape"]), why=R.REFUSED_TAPS["why"],
                                   longest_trainable_kernel={f"F1={F1}": R.conv1_sumsq_max_taps(F1) for F1 in (2, 4, 8)}),
        "row beyond the LDS tiles": dict(shape=list(R.REFUSED_ROW["shape"]), why=R.REFUSED_ROW["why"], largest_T_plus_k1=R.ROW_TILE_MAX),
    }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu-record", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = dict(bounds=dict(dwconv1d_y_dx=R.DW_Y_TOL, dwconv1d_dw=R.DW_DW_TOL, conv1_sumsq_value=R.SUMSQ_TOL,
                           conv1_sumsq_gradient=R.SUMSQ_GRAD_TOL, lag_sums_and_gram_of_largest_entry=R.LAG_TOL,
                           chan_contract_of_scale=R.CC_TOL, model_of_scale=R.MODEL_TOL,
                           widened_by_the_fp32_torch_rule=[]),
               reference="float64 torch on the CPU; errors are max |got - ref| / max |ref|", rows=rows())
    if a.gpu_record:
        with open(a.gpu_record) as f:
            rec = json.load(f)["gpu_rows"]
        worst = {}
        for table, rows_ in rec.items():
            for row, fields in rows_.items():
                dst = out["rows"][table][row]
                errs = {k: v for k, v in fields.items() if isinstance(v, dict) and "error" in v}
                dst["mi355x"] = dict(errors=errs, **{k: v for k, v in fields.items() if k not in errs and k != "route"})
                top = max(errs.items(), key=lambda kv: kv[1]["error"] / kv[1]["bound"])
                dst["mi355x"]["worst"] = dict(tensor=top[0], error_over_bound=top[1]["error"] / top[1]["bound"])
                if top[1]["error"] / top[1]["bound"] > worst.get(table, (0.0,))[0]:
                    worst[table] = (top[1]["error"] / top[1]["bound"], row, top[0])
        missing = [(t, r) for t, rows_ in out["rows"].items() if t != "refusals" for r in rows_ if "mi355x" not in rows_[r]]
        assert not missing, f"rows without a GPU record: {missing}"
        out["worst_observed_over_bound"] = {t: dict(error_over_bound=v[0], row=v[1], tensor=v[2]) for t, v in worst.items()}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
    else:
        json.dump(out, sys.stdout, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
