"""Timing of the saliency of the gated mixture (not a test): utils.saliency.input_saliency with explain="gated" and explain="sbm",
and one training step (forward + loss + backward) of the same InterpGN (FCN expert), at the benchmark shape B=256, T=1000, C=122,
3 classes.  The "gated" call adds the FCN expert's forward and its input-only backward (ign_clconv_dgrad_input* at the end) to
the "sbm" call; its per-kernel launch counts and device times are recorded with it.  Warm-up, then the median of repeated
event-timed runs; every GPU step is a child process under its own time limit, and nothing more is started after one fails.

    python tests/diag_fcn_input_grad.py [--out profiles/fcn_input_grad_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
WARMUP, RUNS = 3, 11
SHAPE = dict(B=256, T=1000, C=122, num_class=3)
KERNELS = ("clconv_fwd", "clconv_dgrad", "clconv_dgrad_input", "clconv_wgrad", "bn_bwd_apply", "bn_relu_pool_bwd", "shp_fwd",
           "shp_bwd", "shp_bwd_x", "instnorm_bwd")


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


def _model():
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from argparse import Namespace
    from models.InterpGN import InterpGN
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, T, C, N = SHAPE["B"], SHAPE["T"], SHAPE["C"], SHAPE["num_class"]
    cfg = Namespace(enc_in=C, seq_len=T, num_class=N, epsilon=1.0, distance_func='euclidean', memory_efficient=False,
                    sbm_cls='linear', dropout=0.0, lambda_reg=0.1, lambda_div=0.1, dnn_type='FCN')
    m = InterpGN(cfg).to(dev)
    x = torch.randn(B, T, C, device=dev)
    y = (torch.arange(B, device=dev) % N)
    m.train()
    with torch.no_grad():
        m(x)                                        # running statistics away from their initial values
    return m, x, y


def step_saliency(explain):
    import torch
    from ign_hip import _lib
    from utils.saliency import input_saliency
    m, x, _ = _model()
    res = _median_ms(lambda: input_saliency(m, x, explain=explain))
    _lib.timing_enable(True)
    input_saliency(m, x, explain=explain)
    res["kernels"] = {}
    for k in KERNELS:
        ms, n = _lib.timing_read(k)
        if n:
            res["kernels"][k] = dict(device_ms=ms, launches=n)
    _lib.timing_enable(False)
    torch.cuda.synchronize()
    return res


def step_train():
    import torch.nn.functional as F
    from ign_hip import ops
    m, x, y = _model()

    def one():
        m.zero_grad(set_to_none=True)
        out, info = m(x)
        ops.backward(F.cross_entropy(out, y) + info.loss.mean() + F.cross_entropy(info.shapelet_preds, y))
    return _median_ms(one)


STEPS = {"saliency_gated": lambda: step_saliency("gated"), "saliency_sbm": lambda: step_saliency("sbm"), "train_step": step_train}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fcn_input_grad_timing.json"))
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(STEPS[a.step]()))
        return
    res = dict(shape=SHAPE)
    for name in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=200)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            res[name] = dict(failed=r.returncode, stderr=r.stderr[-2000:])
            print(name, "FAILED", r.returncode, r.stderr[-2000:], flush=True)
            break                                   # nothing more is started on the GPU after a failed step
        res[name] = json.loads(line[-1][7:])
        print(name, json.dumps(res[name]), flush=True)
    if all(isinstance(res.get(k), dict) and "median_ms" in res[k] for k in STEPS):
        res["gated_over_sbm"] = res["saliency_gated"]["median_ms"] / res["saliency_sbm"]["median_ms"]
        res["gated_over_train_step"] = res["saliency_gated"]["median_ms"] / res["train_step"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
