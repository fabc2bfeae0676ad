"""Cost of the on-device EEG preprocessing (not a test): at B=256, Cin=122, Tin=2000 -> Tout=1000 (q=2) the median of event-timed runs
of ops.eeg_preprocess with 41 taps (decimate only), 207 (band=8:40) and 413 (band=4:40), beside three yardsticks:
  (a) ops.standardise_nct_to_btc on an already decimated (256, 122, 1000) batch -- the floor: those two passes are still needed;
  (b) the torch composition on the device: pad, depthwise F.conv1d(stride=q), mean / std, transpose;
  (c) Experiment.train_one_epoch ms/step on CHISCO-contract shards: (122, 1000) shards without the flag against (122, 2000) shards
      with --eeg_preprocess band=8:40,decimate=2 -- the same model shape; the filter runs on the prefetch stream but shares the
      VALUs with the shapelet kernels, and the raw batch it copies is twice as large.
Bytes moved and FMAs (B*C*Td*M) are computed from the shapes and set against the HBM peak (8.0 TB/s spec) and the fp32 vector rate
of plain v_fmac_f32 (78.6 TFLOP/s = 39.3e12 FMA/s: half the 157.3 TFLOP/s spec, which counts packed FMAs).
Every GPU step is a child process under its own time limit, and nothing more is started after one fails.  No pass / fail threshold.

    python tests/diag_eeg_preprocess.py [--out profiles/eeg_preprocess.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
WARMUP, RUNS = 5, 41
SHAPE = dict(B=256, Cin=122, Tin=2000, q=2, Cout=122, Tout=1000)
SPECS = {41: "decimate=2", 207: "band=8:40,decimate=2", 413: "band=4:40,decimate=2"}
HBM_PEAK, FMA_PEAK = 8.0e12, 39.3e12
HARNESS_N = 1096                       # 768 training samples: three full batches of 256 per epoch
HARNESS_SPEC = SPECS[207]


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


def _counts(M):
    """bytes over HBM and FMAs of one ops.eeg_preprocess call, from the shapes"""
    B, C, Tin, q, Tout = SHAPE["B"], SHAPE["Cin"], SHAPE["Tin"], SHAPE["q"], SHAPE["Tout"]
    Td = -(-Tin // q)
    Tv = min(Td, Tout)
    raw, line, out = 4 * B * C * Tin, 4 * B * C * Tv, 4 * B * Tout * SHAPE["Cout"]
    return dict(bytes=raw + 2 * line + out, bytes_raw_read=raw, bytes_workspace_write_plus_read=2 * line, bytes_out_write=out,
                fmas=B * C * Td * M)


def _torch_composition(x, w, q, R):
    """the same rule from torch ops: reflect pad, depthwise strided convolution (symmetric taps: correlation = convolution),
    per-row statistics, transpose"""
    import torch
    import torch.nn.functional as F
    f = F.conv1d(F.pad(x, (R, R), mode="reflect"), w, stride=q, groups=x.shape[1])
    m = f.mean(dim=2, keepdim=True)
    s = f.std(dim=2, unbiased=True, keepdim=True)
    return ((f - m) / (s + 1e-8)).transpose(1, 2).contiguous()


def _taps(M):
    from utils import eeg_filter as F
    r = F.resolve(SPECS[M], SHAPE["Cin"], SHAPE["Tin"])
    assert len(r.taps) == M and r.Tout == SHAPE["Tout"], (M, len(r.taps), r.Tout)
    return r


def step_kernel():
    import numpy as np
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, C, Tin, q = SHAPE["B"], SHAPE["Cin"], SHAPE["Tin"], SHAPE["q"]
    x = torch.randn(B, C, Tin, device=dev) * 30 + 500
    xd = torch.randn(B, C, SHAPE["Tout"], device=dev) * 30 + 500
    res = dict(hbm_peak_bytes_per_s=HBM_PEAK, fma_peak_per_s=FMA_PEAK)
    floor = _median_ms(lambda: ops.standardise_nct_to_btc(xd))
    floor["bytes"] = 3 * xd.numel() * 4                      # two reads of the batch (L2 / Infinity Cache may serve the second), one write
    res["standardise_decimated_batch"] = floor
    for M in SPECS:
        r = _taps(M)
        h = torch.from_numpy(r.taps.astype(np.float32)).to(dev)
        k = _median_ms(lambda: ops.eeg_preprocess(x, h, decimate=q, edge=r.edge))
        k.update(_counts(M))
        sec = k["median_ms"] * 1e-3
        k["share_of_hbm_peak"] = k["bytes"] / sec / HBM_PEAK
        k["share_of_fma_peak"] = k["fmas"] / sec / FMA_PEAK
        k["over_floor"] = k["median_ms"] / floor["median_ms"]
        res[f"eeg_preprocess_M{M}"] = k
        w = h.view(1, 1, M).repeat(C, 1, 1).contiguous()
        t = _median_ms(lambda: _torch_composition(x, w, q, (M - 1) // 2))
        t["over_eeg_preprocess"] = t["median_ms"] / k["median_ms"]
        res[f"torch_composition_M{M}"] = t
        got, _ = ops.eeg_preprocess(x, h, decimate=q, edge=r.edge)
        res[f"max_abs_diff_to_torch_M{M}"] = float((got - _torch_composition(x, w, q, (M - 1) // 2)).abs().max())
    return res


def _harness(preprocess):
    import numpy as np
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    import run as ign_run
    import tempfile
    from exp.experiment_classification import Experiment
    T = SHAPE["Tin"] if preprocess else SHAPE["Tout"]
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(0)
        X = np.lib.format.open_memmap(os.path.join(tmp, "X.npy"), mode="w+", dtype=np.float32, shape=(HARNESS_N, SHAPE["Cin"], T))
        for i in range(0, HARNESS_N, 64):
            X[i:i + 64] = rng.standard_normal((min(64, HARNESS_N - i), SHAPE["Cin"], T), dtype=np.float32) * 30 + 500
        X.flush()
        del X
        np.save(os.path.join(tmp, "y.npy"), rng.integers(0, 39, size=HARNESS_N))
        argv = ["--model", "InterpGN", "--dnn_type", "FCN", "--data", "EEG3", "--data_root", tmp, "--dataset", "chisco_npy",
                "--batch_size", str(SHAPE["B"]), "--amp", "--train_epochs", "4", "--num_workers", "0", "--seed", "0"]
        a = ign_run.get_args(argv + (["--eeg_preprocess", HARNESS_SPEC] if preprocess else []))
        os.chdir(tmp)
        try:
            ign_run.set_seed(0)
            exp = Experiment(a)
            assert (a.seq_len, a.enc_in) == (SHAPE["Tout"], SHAPE["Cout"])
            n = len(exp.train_loader)
            _, ts = exp.train_one_epoch(0, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for e in (1, 2, 3):
                losses, ts = exp.train_one_epoch(e, ts)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            os.chdir(cwd)
    return dict(eeg_preprocess=HARNESS_SPEC if preprocess else "none", shard_shape=[HARNESS_N, SHAPE["Cin"], T],
                ms_per_step=1e3 * dt / (3 * n), steps_timed=3 * n, last_loss=float(losses[-1]))


STEPS = {"kernel": step_kernel, "harness_step_plain": lambda: _harness(False), "harness_step_preprocessed": lambda: _harness(True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eeg_preprocess.json"))
    a = ap.parse_args()
    if a.step:
        res = STEPS[a.step]()
        print("RESULT " + json.dumps(res))
        return
    res = dict(shape=SHAPE, specs={str(k): v for k, v in SPECS.items()})
    for name in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=300)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            res[name] = dict(failed=r.returncode, stderr=r.stderr[-2000:])
            break                                   # nothing more is started on the GPU after a failed step
        res[name] = json.loads(line[-1][7:])
        print(name, json.dumps(res[name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    if any("failed" in v for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
