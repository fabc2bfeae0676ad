"""Cost of mixup / CutMix (not a test), at the benchmark shape (B=256, C=122, T=1000), medians of event-timed runs:
  * ops.mix -- mixup, CutMix, both, a ragged batch -- beside x.clone() of the same batch in the same process.  The mix moves three
    streams (two reads, one write) against the clone's two; bytes moved over time are given as a share of the HBM peak (8.0 TB/s
    spec, MI355X; about 6.3 TB/s is achievable by a plain copy);
  * the soft-label loss tail (ops.ign_loss with y_b / lam) beside the weighted tail it extends, at N = 3 and N = 39 classes,
    B = 256: forward launch only (both are single-block kernels of a few microseconds, so the timed region is launch-bound);
  * in two further processes: the harness step (Experiment.train_one_epoch on --data SYNTH, per-step H2D copy and host draws
    included) without and with --mix mixup=0.4.
Every GPU step is a child process under its own time limit, and nothing more is started after one fails.  No pass / fail threshold.

    python tests/diag_mix.py [--out profiles/mix.json]         # written as the file's `diag` entry
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


def step_kernel():
    import numpy as np
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    from utils.mix import MixSpec, mix_draws
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, C, T = SHAPE["B"], SHAPE["C"], SHAPE["T"]
    x = torch.randn(B, T, C, device=dev)
    one = x.numel() * 4
    res = dict(bytes_per_stream=one, hbm_peak_bytes_per_s=HBM_PEAK)
    put = lambda a: torch.from_numpy(a).to(dev)

    def draws(spec, lens):
        roll, lam, span = mix_draws(12345, B, lens, spec)
        return put(lam), roll, put(span)
    lam_m, roll_m, _ = draws(MixSpec(mixup=0.4), T)
    lam_c, roll_c, span_c = draws(MixSpec(cutmix=1.0), T)
    lam_b, roll_b, span_b = draws(MixSpec(mixup=0.4, cutmix=1.0), T)
    lens_h = np.random.default_rng(0).integers(T // 2, T + 1, B)
    lam_r, roll_r, span_r = draws(MixSpec(mixup=0.4, cutmix=1.0), lens_h)
    lens = put(lens_h.astype(np.int32))
    cases = {
        "clone": (2, lambda: x.clone()),
        "mix_mixup": (3, lambda: ops.mix(x, lam_m, roll_m)),
        "mix_cutmix": (3, lambda: ops.mix(x, lam_c, roll_c, span=span_c)),
        "mix_both": (3, lambda: ops.mix(x, lam_b, roll_b, span=span_b)),
        "mix_both_ragged": (3, lambda: ops.mix(x, lam_r, roll_r, span=span_r, lengths=lens)),
        "clone_again": (2, lambda: x.clone()),
    }
    for name, (streams, fn) in cases.items():
        r = _median_ms(fn)
        r["streams"] = streams
        r["share_of_hbm_peak"] = streams * one / (r["median_ms"] * 1e-3) / HBM_PEAK
        res[name] = r
    for name in cases:
        if name.startswith("mix"):
            res[name]["ratio_to_clone"] = res[name]["median_ms"] / res["clone"]["median_ms"]
    return res


def step_loss_tail():
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    dev = torch.device("cuda:0")
    B = SHAPE["B"]
    res = dict(B=B)
    for N in (3, 39):
        g = torch.Generator().manual_seed(N)
        s, d = (torch.randn(B, N, generator=g) * 3).to(dev), (torch.randn(B, N, generator=g) * 3).to(dev)
        ya, yb = torch.randint(0, N, (B,), generator=g).to(dev), torch.randint(0, N, (B,), generator=g).to(dev)
        lam, w = torch.rand(B, generator=g).to(dev), (0.2 + 4.8 * torch.rand(N, generator=g)).to(dev)
        reg = torch.zeros(1, device=dev)
        hard = _median_ms(lambda: ops.ign_loss(s, d, ya, 0.5, reg=reg, class_weight=w, label_smoothing=0.1))
        soft = _median_ms(lambda: ops.ign_loss(s, d, ya, 0.5, reg=reg, class_weight=w, label_smoothing=0.1, y_b=yb, lam=lam))
        res[f"N{N}"] = dict(weighted_tail=hard, soft_label_tail=soft, ratio=soft["median_ms"] / hard["median_ms"])
    return res


def _harness(mix):
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    import run as ign_run
    import tempfile
    from exp.experiment_classification import Experiment
    argv = ["--model", "InterpGN", "--dnn_type", "FCN", "--data", "SYNTH", "--synthetic", f"{HARNESS_N},122,1000,3", "--dataset",
            "SYNTH", "--batch_size", str(SHAPE["B"]), "--amp", "--train_epochs", "3", "--num_workers", "0", "--seed", "0"]
    a = ign_run.get_args(argv + (["--mix", mix] if mix else []))
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
    return dict(mix=mix or "none", ms_per_step=1e3 * dt / (2 * n), steps_timed=2 * n, last_loss=float(losses[-1]))


STEPS = {"kernel": step_kernel, "loss_tail": step_loss_tail, "harness_step_plain": lambda: _harness(None),
         "harness_step_mixup": lambda: _harness("mixup=0.4")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix.json"))
    a = ap.parse_args()
    if a.step:
        res = STEPS[a.step]()
        print("RESULT " + json.dumps(res))
        return
    res = dict(shape=SHAPE)
    for name in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=300)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            res[name] = dict(failed=r.returncode, stderr=r.stderr[-2000:])
            break                                   # nothing more is started on the GPU after a failed step
        res[name] = json.loads(line[-1][7:])
        print(name, json.dumps(res[name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}      # the file's other entries (parity, bench) are kept
    doc["diag"] = res
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    if any("failed" in v for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
