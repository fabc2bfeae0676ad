"""Cost of the regression loss tail: the fused HIP launch (ops.crps_loss / ops.ign_crps_loss, forward + gradient) against the
torch composite it replaces (softmax, cumsum, compare, square, sums, the gini gate and their autograd), at N = 10 bins.
A measuring script, not a test.

    python tests/diag_crps.py [--steps 200] [--json results.json]
Prints one line per (op, B): median device time per call (CUDA events around each call, launch overhead included) and the
device kernels one call launches (torch.profiler)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _time(fn, steps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(steps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def _launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA")
               and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import speech_imagery_eeg_amd  # noqa: F401
    from exp.experiment_regression import CRPSLoss
    from ign_hip import ops
    dev = torch.device("cuda:0")
    N = 10
    e = torch.linspace(-2, 2, N + 1, dtype=torch.float64)
    e[-1] = float("inf")
    edges = e[1:].to(dev)
    crps_t = CRPSLoss(edges)
    unit = ops.unit_grad(dev)
    rows = []
    for B in (32, 256):
        g = torch.Generator().manual_seed(B)
        s = (torch.randn(B, N, generator=g) * 2).to(dev).requires_grad_(True)
        d = (torch.randn(B, N, generator=g) * 2).to(dev).requires_grad_(True)
        y = torch.randn(B, generator=g).to(dev)
        reg = torch.tensor([0.25], device=dev)

        def fused_crps():
            torch.autograd.grad(ops.crps_loss(s, y, edges), [s], grad_outputs=unit)

        def torch_crps():
            torch.autograd.grad(crps_t(s, y), [s])

        def fused_ign():
            torch.autograd.grad(ops.ign_crps_loss(s, d, y, edges, 1.0, reg=reg)[0], [s, d], grad_outputs=unit)

        def torch_ign():
            q = torch.softmax(s, -1)
            eta = ((q * q).sum(-1, keepdim=True) * N - 1) / (N - 1)
            out = eta * s + (1 - eta) * d
            torch.autograd.grad(crps_t(out, y) + reg.sum() + 1.0 * crps_t(s, y), [s, d])

        for name, fn in (("crps fused", fused_crps), ("crps torch", torch_crps), ("ign tail fused", fused_ign),
                         ("ign tail torch", torch_ign)):
            r = {"op": name, "B": B, "N": N, "us_per_call": round(_time(fn, args.steps), 2), "launches": _launches(fn)}
            rows.append(r)
            print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
