"""Cost of the zero-phase IIR stage (not a test): at the CHISCO shape B=256, C=122, T=1651, the median of event-timed runs of
ops.eeg_iir (ign_eeg_iir_nct) for the one-section notch and for the five-section chain hp=0.5,lp=40,order=4,notch=50, beside the
launches the stage sits between on the prefetch stream, ops.standardise_nct_to_btc and ops.eeg_filterbank (band=8:30, default
taps), timed in the same process.  Float64 multiply-adds are counted from the shapes (5 per sample, section and direction over the
N = T + 2P extended row, twice over for the second run of every chunk) and set against the vector float64 peak; bytes over HBM (one
read and one write of the batch) against the HBM peak.  The stage must hide behind the step it runs beside: the five-section
median is set against one tenth of the headline step of profiles/r3_bench_line.json.  The GPU step is a child process under its
own time limit.

    python tests/diag_eeg_iir.py [--bench profiles/r3_bench_line.json] [--out profiles/eeg_iir.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
WARMUP, RUNS = 5, 41
SHAPE = dict(B=256, C=122, T=1651)
SPECS = {"notch": "notch=50", "chain5": "hp=0.5,lp=40,order=4,notch=50"}
HBM_PEAK, VALU_F64_PEAK = 8.0e12, 78.6e12


def _median_ms(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return dict(median_ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1], runs=RUNS, warmup=WARMUP)


def step_kernel():
    import numpy as np
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    from utils.eeg_filter import parse_eeg_preprocess, resolve
    from utils.eeg_iir import iir_numpy, resolve_iir
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, C, T = SHAPE["B"], SHAPE["C"], SHAPE["T"]
    x = torch.randn(B, C, T, device=dev) * 30 + torch.empty(B, C, 1, device=dev).uniform_(-2e4, 2e4)
    y = torch.empty(B, C, T, device=dev)
    res = dict(hbm_peak_bytes_per_s=HBM_PEAK, valu_f64_peak_flop_per_s=VALU_F64_PEAK)
    pre = resolve(parse_eeg_preprocess("band=8:30"), C, T, notice=None)
    taps = torch.as_tensor(pre.taps2d, dtype=torch.float32).to(dev)
    kw = dict(decimate=pre.q, edge=pre.edge, channels=pre.Cout, timepoints=pre.Tout)
    res["standardise_first"] = _median_ms(lambda: ops.standardise_nct_to_btc(x))
    res["filterbank_band_8_30"] = dict(_median_ms(lambda: ops.eeg_filterbank(x, taps, None, **kw)), taps=int(taps.shape[1]))
    for name, spec in SPECS.items():
        st = resolve_iir(spec, T)
        coef = torch.from_numpy(st.table).to(dev)
        k = _median_ms(lambda: ops.eeg_iir(x, coef, pad=st.pad, g0=st.g0, out=y))
        N = T + 2 * st.pad
        fma = 2 * (B * C) * N * st.ns * 5 * 2                          # directions x rows x samples x sections x 5, run twice
        nbytes = 2 * 4 * B * C * T
        sec = k["median_ms"] * 1e-3
        k.update(spec=spec, sections=st.ns, pad=st.pad, f64_fma=fma, bytes=nbytes, lds_bytes_per_row=8 * N,
                 share_of_f64_valu_peak=2 * fma / sec / VALU_F64_PEAK, share_of_hbm_peak=nbytes / sec / HBM_PEAK)
        k["two_calls_bitwise"] = bool(torch.equal(ops.eeg_iir(x, coef, pad=st.pad, g0=st.g0), y))
        rows = y[:2, :3].cpu().numpy()                                 # six rows against the float64 rule, at the row's scale
        ref = iir_numpy(x[:2, :3].cpu().numpy(), st.table, st.pad, st.g0)
        xs = x[:2, :3].double().cpu().numpy()
        scale = np.abs(xs - xs[..., :1]).max(axis=-1, keepdims=True)
        k["max_err_over_row_scale_beyond_one_fp32_rounding"] = float(
            (np.maximum(np.abs(rows - ref) - 2.0 ** -23 * np.abs(ref), 0.0) / scale).max())
        res[f"eeg_iir_{name}"] = k
    res["standardise_last"] = _median_ms(lambda: ops.standardise_nct_to_btc(x))
    std = min(res["standardise_first"]["median_ms"], res["standardise_last"]["median_ms"])
    for name in SPECS:
        res[f"{name}_over_standardise"] = res[f"eeg_iir_{name}"]["median_ms"] / std
        res[f"{name}_over_filterbank"] = res[f"eeg_iir_{name}"]["median_ms"] / res["filterbank_band_8_30"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"])
    ap.add_argument("--bench", default=os.path.join(ROOT, "profiles", "r3_bench_line.json"),
                    help="a file holding bench.py's JSON result line: the step the stage runs beside")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eeg_iir.json"))
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step_kernel()))
        return
    res = dict(shape=SHAPE, specs=SPECS,
               yardstick="the launch runs on the prefetch stream between ign_eeg_spatial_nct and the FIR / standardisation launch and "
                         "must hide behind the training step it overlaps with: five-section median < bench_step_ms / 10")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "kernel"], capture_output=True, text=True, timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        res["kernel"] = dict(failed=r.returncode, stderr=r.stderr[-2000:])
    else:
        res["kernel"] = json.loads(line[-1][7:])
        print("kernel", json.dumps(res["kernel"]), flush=True)
        if a.bench and os.path.exists(a.bench):
            b = json.load(open(a.bench))
            step = b.get("ms_per_step")
            if step:
                res["bench_step_ms"], res["budget_ms"] = step, step / 10.0
                res["chain5_over_budget"] = res["kernel"]["eeg_iir_chain5"]["median_ms"] / (step / 10.0)
                res["hides_behind_the_step"] = bool(res["chain5_over_budget"] < 1.0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    if "failed" in res["kernel"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
