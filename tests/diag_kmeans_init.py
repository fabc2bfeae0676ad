"""Cost of the k-means shapelet initialisation (not a test): at the benchmark shape (B=256, C=122, T=1000, four groups of K=5 with
L = 100 / 200 / 300 / 500), in one process, one Lloyd step per group (ops.shapelet_kmeans_step, split by kernel through the timing
registry) beside the bank forward and weight-gradient pass of the same groups (MSE distance: the arithmetic the Lloyd step shares);
and, in a second process, the wall time of kmeans_init_ at its defaults (10 iterations x 8 batches) on the SBM of those groups.
Warm-up, then the median of repeated event-timed runs; every GPU step is a child process under its own time limit, and nothing
more is started after one fails.  No pass / fail threshold: the initialisation runs once per training.

    python tests/diag_kmeans_init.py [--out profiles/kmeans_init.json]
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
WARMUP, RUNS = 5, 21
SHAPE = dict(B=256, C=122, T=1000, K=5, L=[100, 200, 300, 500])
KERNELS = ("kmeans_assign", "kmeans_accum", "kmeans_reduce")


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


def step_kernels():
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, C, T, K, Ls = SHAPE["B"], SHAPE["C"], SHAPE["T"], SHAPE["K"], SHAPE["L"]
    xn, _ = ops.instance_norm(torch.randn(B, T, C, device=dev))
    # centroids as k-means leaves them: data windows, not noise
    ws = [torch.stack([xn[k, :, 7 * k:7 * k + L] for k in range(K)]).contiguous() for L in Ls]
    res = dict(element_ops=sum(B * C * K * (T - L + 1) * L for L in Ls), lloyd_step={}, lloyd_kernels_ms={})
    for L, w in zip(Ls, ws):
        res["lloyd_step"][str(L)] = _median_ms(lambda: ops.shapelet_kmeans_step(xn, w))
    res["lloyd_step_all_groups_ms"] = sum(v["median_ms"] for v in res["lloyd_step"].values())
    _lib.timing_enable(True)
    for w in ws:
        ops.shapelet_kmeans_step(xn, w)
    torch.cuda.synchronize()
    for name in KERNELS:
        res["lloyd_kernels_ms"][name] = _lib.timing_read(name)[0]
    _lib.timing_enable(False)
    mode = ops.DIST_MSE | ops.GATE_RBF
    bank = ops._Bank(xn, ws, [None] * len(Ls), 1.0, mode, [1] * len(Ls), True)
    P, D = ops._bank_fwd(bank, xn)
    gP = torch.randn(P.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    res["bank_forward"] = _median_ms(lambda: ops._bank_fwd(bank, xn))
    res["bank_weight_pass"] = _median_ms(lambda: ops._bank_wgrad(bank, xn, gP, P, D))
    res["bank_forward_plus_weight_pass_ms"] = res["bank_forward"]["median_ms"] + res["bank_weight_pass"]["median_ms"]
    res["lloyd_over_forward_plus_weight_pass"] = res["lloyd_step_all_groups_ms"] / res["bank_forward_plus_weight_pass_ms"]
    return res


def step_full_init():
    import torch
    from argparse import Namespace
    import speech_imagery_eeg_amd  # noqa: F401
    from models.Shapelet import ShapeBottleneckModel
    from utils.shapelet_init import kmeans_init_
    dev = torch.device("cuda:0")
    B, C, T, K, Ls = SHAPE["B"], SHAPE["C"], SHAPE["T"], SHAPE["K"], SHAPE["L"]
    cfg = Namespace(enc_in=C, seq_len=T, num_class=3, epsilon=1.0, distance_func='euclidean', memory_efficient=False,
                    sbm_cls='linear', dropout=0.0, lambda_reg=0.1, lambda_div=0.1)
    torch.manual_seed(0)
    model = ShapeBottleneckModel(cfg, [K] * len(Ls), [L / T for L in Ls]).to(dev)
    batches = [(torch.randn(B, T, C, device=dev),) for _ in range(8)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rep = kmeans_init_(model, batches)                   # the defaults: 10 iterations, 8 batches
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return dict(wall_s=wall, iters=rep["iters"], batches=rep["batches"], windows_per_channel=rep["windows"],
                groups=[dict(length=g["length"], inertia=g["inertia"], empty=g["empty"]) for g in rep["groups"]])


STEPS = {"lloyd_vs_bank": step_kernels, "kmeans_init_defaults": step_full_init}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_init.json"))
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(STEPS[a.step]()))
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
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    if any("failed" in v for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
