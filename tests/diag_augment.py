"""Cost of the on-device augmentation (not a test): at the benchmark shape (B=256, C=122, T=1000) the median of event-timed runs of
ops.augment -- everything on, everything but the noise, shift only -- beside two yardsticks: x.clone() of the same batch (the
out-of-place memory floor: one read, one write) and the torch composition that produces the same transforms (roll, rand / randn_like,
mul, add, two mask multiplies).  Bytes moved over time are given as a share of the HBM peak (8.0 TB/s spec, MI355X).  In a second and
third process: the harness step (Experiment.train_one_epoch on --data SYNTH, per-step H2D copy included) without and with --augment.
Every GPU step is a child process under its own time limit, and nothing more is started after one fails.  No pass / fail threshold.

    python tests/diag_augment.py [--out profiles/augment.json]
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
SHAPE = dict(B=256, C=122, T=1000)
HBM_PEAK = 8.0e12
RATES = dict(shift=0.1, scale=0.1, channel_drop=0.1, time_mask=0.1)
SIGMA = 0.05
AUG = "shift=0.1,scale=0.1,noise=0.05,chan_drop=0.1,time_mask=0.1"
HARNESS_N = 2048                       # SYNTH samples on the host (1 GB): 8 steps per epoch at B = 256


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


def _torch_composition(x, noise):
    """the same transforms from torch ops (its own random numbers): one roll per batch (a per-sample shift would need a gather),
    per-(b, c) gain and electrode mask, one span per sample, Gaussian noise"""
    import torch
    B, T, C = x.shape
    dev = x.device
    y = torch.roll(x, int(torch.randint(-T // 10, T // 10 + 1, (1,)).item()), dims=1)
    y = y * (1 + 0.1 * (2 * torch.rand(B, 1, C, device=dev) - 1))
    if noise:
        y = y + SIGMA * torch.randn_like(y)
    y = y * (torch.rand(B, 1, C, device=dev) >= 0.1)
    start = torch.randint(0, T - T // 10, (B, 1, 1), device=dev)
    t = torch.arange(T, device=dev).view(1, T, 1)
    return y * ~((t >= start) & (t < start + T // 10))


def step_kernel():
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, C, T = SHAPE["B"], SHAPE["C"], SHAPE["T"]
    x = torch.randn(B, T, C, device=dev)
    traffic = 2 * x.numel() * 4
    res = dict(bytes_read_plus_written=traffic, hbm_peak_bytes_per_s=HBM_PEAK)
    cases = {
        "augment_all": lambda: ops.augment(x, 12345, noise=SIGMA, **RATES),
        "augment_all_but_noise": lambda: ops.augment(x, 12345, **RATES),
        "augment_shift_only": lambda: ops.augment(x, 12345, shift=0.1),
        "augment_noise_only": lambda: ops.augment(x, 12345, noise=SIGMA),
        "clone": lambda: x.clone(),
        "torch_composition_all": lambda: _torch_composition(x, True),
        "torch_composition_all_but_noise": lambda: _torch_composition(x, False),
    }
    for name, fn in cases.items():
        r = _median_ms(fn)
        r["share_of_hbm_peak"] = traffic / (r["median_ms"] * 1e-3) / HBM_PEAK
        res[name] = r
    # a ragged batch costs no more: lengths uniform in T/2 .. T
    lens = torch.randint(T // 2, T + 1, (B,), device=dev, dtype=torch.int32)
    res["augment_all_ragged"] = _median_ms(lambda: ops.augment(x, 12345, lengths=lens, noise=SIGMA, **RATES))
    return res


def _harness(augment):
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    import run as ign_run
    import tempfile
    from exp.experiment_classification import Experiment
    argv = ["--model", "InterpGN", "--dnn_type", "FCN", "--data", "SYNTH", "--synthetic", f"{HARNESS_N},122,1000,3", "--dataset",
            "SYNTH", "--batch_size", str(SHAPE["B"]), "--amp", "--train_epochs", "3", "--num_workers", "0", "--seed", "0"]
    a = ign_run.get_args(argv + (["--augment", AUG] if augment else []))
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            ign_run.set_seed(0)
            exp = Experiment(a)
            n = len(exp.train_loader)
            _, ts = exp.train_one_epoch(0, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for e in (1, 2):
                losses, ts = exp.train_one_epoch(e, ts)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            os.chdir(cwd)
    return dict(augment=AUG if augment else "none", ms_per_step=1e3 * dt / (2 * n), steps_timed=2 * n,
                last_loss=float(losses[-1]))


STEPS = {"kernel": step_kernel, "harness_step_plain": lambda: _harness(False), "harness_step_augmented": lambda: _harness(True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment.json"))
    a = ap.parse_args()
    if a.step:
        res = STEPS[a.step]()
        print("RESULT " + json.dumps(res))
        return
    res = dict(shape=SHAPE, rates=dict(RATES, noise=SIGMA))
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
