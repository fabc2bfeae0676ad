"""Timing of the input-gradient pass (not a test): ign_shapelet_bwd_input_bank against ign_shapelet_bwd_bank at the benchmark
shape (C=122, T=1000, B=256, four groups of K=5 with L = 100 / 200 / 300 / 500; both passes do E = 1.11e11 element-ops), and
ign_instnorm_bwd against ign_instnorm_fwd.  Warm-up, then the median of repeated event-timed runs; every GPU step is a child
process under its own time limit, and nothing more is started after one fails.

    python tests/diag_input_grad.py [--out profiles/input_grad.json] [--bench-line parent|this FILE ...]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
WARMUP, RUNS = 5, 21


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


def step_bank(mode):
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, C, T, K, Ls = 256, 122, 1000, 5, (100, 200, 300, 500)
    xn, _ = ops.instance_norm(torch.randn(B, T, C, device=dev))
    ws = [torch.randn(K, C, L, device=dev) for L in Ls]
    thrs = [torch.rand(1, K, C, device=dev) for _ in Ls] if mode & ops.GATE_LTS else [None] * len(Ls)
    bank = ops._Bank(xn, ws, thrs, 1.0, mode, [1] * len(Ls), True)
    P, D = ops._bank_fwd(bank, xn)
    gP = torch.randn_like(P)
    E = sum(B * C * K * (T - L + 1) * L for L in Ls)
    w = _median_ms(lambda: ops._bank_wgrad(bank, xn, gP, P, D))
    x = _median_ms(lambda: ops._bank_xgrad(bank, xn, gP, P, D))
    return dict(element_ops=E, weight_pass=w, input_pass=x, input_over_weight=x["median_ms"] / w["median_ms"],
                input_pass_Telem_per_s=E / x["median_ms"] / 1e9, weight_pass_Telem_per_s=E / w["median_ms"] / 1e9)


def step_instnorm():
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, T, C = 256, 1000, 122
    x = torch.randn(B, T, C, device=dev) * 3 + 50
    g = torch.randn(B, C, T, device=dev)
    gx = torch.empty_like(x)
    L = _lib.lib()
    f = _median_ms(lambda: ops.instance_norm(x))
    b = _median_ms(lambda: _lib.check(L.ign_instnorm_bwd(ops._ptr(x), ops._ptr(g), ops._ptr(gx), B, T, C, 1e-8, ops._stream()),
                                      "ign_instnorm_bwd"))
    return dict(forward=f, backward=b, backward_over_forward=b["median_ms"] / f["median_ms"])


STEPS = {"bank_l1_rbf": lambda: step_bank(0x00), "bank_mse_lts": lambda: step_bank(0x11), "instnorm": step_instnorm}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_grad.json"))
    ap.add_argument("--bench-line", nargs=2, action="append", default=[], metavar=("LABEL", "FILE"),
                    help="record the JSON result line of a bench.py run (its last line starting with '{') under LABEL")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(STEPS[a.step]()))
        return
    res = dict(shape=dict(B=256, C=122, T=1000, K=5, L=[100, 200, 300, 500]))
    for name in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=300)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            res[name] = dict(failed=r.returncode, stderr=r.stderr[-2000:])
            break                                   # nothing more is started on the GPU after a failed step
        res[name] = json.loads(line[-1][7:])
        print(name, json.dumps(res[name]), flush=True)
    for label, path in a.bench_line:
        lines = [l for l in open(path).read().splitlines() if l.startswith("{")]
        res.setdefault("bench", {}).setdefault(label, []).append(json.loads(lines[-1]) if lines else None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
