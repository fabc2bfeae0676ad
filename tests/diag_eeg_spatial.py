"""Cost of the spatial filter stage (not a test): at the CHISCO shape B=256, Cin=122, T=1000, Cs=122, for G=1 and G=4, the median of
event-timed runs of ops.eeg_spatial (ign_eeg_spatial_nct) and ops.eeg_gram (ign_eeg_gram_nct), beside the launch the stage sits
next to on the prefetch stream, ops.standardise_nct_to_btc at the same shape, timed in the same process.  FLOPs (2*B*Cs*Cin*T for
the apply; B*C*C*T for the Gram's computed triangle of 64 x 64 tiles counted from the tile table, 2 per multiply-add) and bytes over
HBM are computed from the shapes and set against the f32 matrix peak (157.3e12 FLOP/s) and the HBM peak (8.0 TB/s spec).  --bench
takes the headline step time of a bench.py result line of the same session (the step the apply launch must hide behind).  The GPU
step is a child process under its own time limit.  No pass / fail threshold.

    python tests/diag_eeg_spatial.py [--bench BENCH_LINE.json] [--out profiles/eeg_spatial.json]
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
SHAPE = dict(B=256, Cin=122, T=1000, Cs=122)
GROUPS = (1, 4)
HBM_PEAK, MFMA_F32_PEAK = 8.0e12, 157.3e12


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


def _rates(k, flops, nbytes):
    sec = k["median_ms"] * 1e-3
    k.update(flops=flops, bytes=nbytes, share_of_f32_matrix_peak=flops / sec / MFMA_F32_PEAK, share_of_hbm_peak=nbytes / sec / HBM_PEAK)
    return k


def step_kernel():
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, Cin, T, Cs = SHAPE["B"], SHAPE["Cin"], SHAPE["T"], SHAPE["Cs"]
    x = torch.randn(B, Cin, T, device=dev) * 30 + torch.empty(B, Cin, 1, device=dev).uniform_(-2e4, 2e4)
    res = dict(hbm_peak_bytes_per_s=HBM_PEAK, f32_matrix_peak_flop_per_s=MFMA_F32_PEAK)
    nt = -(-Cs // 64)
    for G in GROUPS:
        W = torch.randn(G, Cs, Cin, device=dev) / Cin ** 0.5
        gid = (torch.arange(B, device=dev) % G).to(torch.int32) if G > 1 else None
        y = torch.empty(B, Cs, T, device=dev)
        gram, count = torch.empty(G, Cs, Cs, device=dev), torch.empty(G, device=dev, dtype=torch.int32)
        std_first = _median_ms(lambda: ops.standardise_nct_to_btc(x))
        apply = _median_ms(lambda: ops.eeg_spatial(x, W, gid, out=y))
        gr = _median_ms(lambda: ops.eeg_gram(y, gid, G, out=(gram, count)))
        std_last = _median_ms(lambda: ops.standardise_nct_to_btc(x))
        res[f"eeg_spatial_G{G}"] = _rates(apply, 2 * B * Cs * Cin * T, 4 * B * T * (Cin + Cs) + 4 * G * Cs * Cin)
        # the Gram computes nt (nt + 1) / 2 tiles of 64 x 64 per sample; it reads y twice per tile pair and moves the per-sample partials
        res[f"eeg_gram_G{G}"] = _rates(gr, 2 * B * (nt * (nt + 1) // 2) * 64 * 64 * T, 4 * B * Cs * T * 2 + 2 * 4 * B * Cs * Cs)
        res[f"standardise_first_G{G}"], res[f"standardise_last_G{G}"] = std_first, std_last
        res[f"apply_over_standardise_G{G}"] = apply["median_ms"] / min(std_first["median_ms"], std_last["median_ms"])
        res[f"two_calls_bitwise_G{G}"] = bool(torch.equal(ops.eeg_spatial(x, W, gid), y))
    return res


def step_cpu_emulation():
    """No device: the numpy fp32 restatement of the rule on the tests' case table (error over each a-priori bound) and, on the tests'
    shards, the distance of the CPU loader path (restatement, then the fp32 numpy rules) from the float64 path, as the largest
    |ref - f64| / (1 + |f64|) -- the figure the prefetcher test's bound is taken from, with its margin of 2."""
    import tempfile
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import eeg_spatial_cases as K
    s = K.S()
    from data_provider.eeg_chain import EEGChain
    from data_provider.eeg_npy import EEGNpyDataset, per_sample_standardise
    from utils.eeg_filter import filterbank_numpy
    res = dict(margin=2.0, apply_cases={}, identity_inexact={}, loader_path={})
    for label in K.APPLY_CASES:
        k = K.apply_case(label)
        r1, r2 = K.check_apply(label, s.spatial_numpy(k["x"], k["W"], k["gid"], dtype=np.float32))
        res["apply_cases"][label] = dict(error_over_bound_1=r1, centred_error_over_bound_2=r2)
        _, exact = K.identity_expectation(k["x"])
        res["identity_inexact"][label] = dict(elements=int((~exact).sum()), of=int(exact.size), rows=int((~exact).any(axis=-1).sum()))
    with tempfile.TemporaryDirectory() as d:
        X, _, _ = K.write_shards(d)
        for spec in ("ref=car", "ref=car,align=euclid"):
            for pre in (None, "band=8:30,taps=41"):
                ds = EEGNpyDataset(d, flag="train", chain=EEGChain(spatial=spec, preprocess=pre))
                if "align" in spec:
                    ds.spatial.W = s.fit_alignment(ds.raw_batches(8), ds.spatial.W0, 3, 1e-6, notice=None)
                worst = 0.0
                for i in range(len(ds)):
                    j = ds.idx[i]
                    v64 = s.spatial_numpy(X[j], ds.spatial.matrix_of(int(ds.group[j])))
                    p = ds.pre
                    f64 = per_sample_standardise(v64).T if pre is None else \
                        filterbank_numpy(v64, p.taps2d.astype(np.float32), None, p.q, p.edge, p.Cout, p.Tout)
                    worst = max(worst, float((np.abs(ds[i][0].numpy() - f64) / (1.0 + np.abs(f64))).max()))
                res["loader_path"][f"{spec} | {pre or 'standardise'}"] = worst
    return res


STEPS = {"cpu_emulation": step_cpu_emulation, "kernel": step_kernel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--bench", default=None, help="a file holding bench.py's JSON result line of the same session")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eeg_spatial.json"))
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(STEPS[a.step]()))
        return
    res = dict(shape=SHAPE, groups=list(GROUPS),
               yardstick="the apply launch runs on the prefetch stream beside ign_standardise_nct_to_btc and must be shorter than the "
                         "training step it hides behind (bench_step_ms)")
    for name in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=300)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            res[name] = dict(failed=r.returncode, stderr=r.stderr[-2000:])
            break                                   # nothing more is started on the GPU after a failed step
        res[name] = json.loads(line[-1][7:])
        print(name, json.dumps(res[name]), flush=True)
    if a.bench and os.path.exists(a.bench):
        lines = [l for l in open(a.bench).read().splitlines() if l.startswith("{")]
        if lines:
            b = json.loads(lines[-1])
            res["bench"] = {k: b[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "warmup") if k in b}
            step = b.get("ms_per_step")
            if step and "kernel" in res and "failed" not in res["kernel"]:
                res["bench_step_ms"] = step
                for G in GROUPS:
                    res[f"apply_over_bench_step_G{G}"] = res["kernel"][f"eeg_spatial_G{G}"]["median_ms"] / step
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    if any("failed" in v for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
