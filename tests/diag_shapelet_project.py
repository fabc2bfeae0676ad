"""Cost of the shapelet projection (not a test): at the benchmark shape (B=256, C=122, T=1000, four groups of K=5 with
L = 100 / 200 / 300 / 500, L1 distance), one ordered pass of project_ over 4 batches resident on the device, per batch, against the
eval-mode ``shapelet_features`` call alone on the same batches -- the forward every projection batch runs anyway -- and the
project-step launches by themselves through the timing registry.  Warm-up, then the median of repeated event-timed runs, in a child
process under its own time limit.  No pass / fail threshold: a projection runs once per training, or once every N epochs.

    python tests/diag_shapelet_project.py [--out profiles/shapelet_project.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
WARMUP, RUNS, BATCHES = 3, 11, 4
SHAPE = dict(B=256, C=122, T=1000, K=5, L=[100, 200, 300, 500])


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


def step_pass():
    import torch
    from argparse import Namespace
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    from models.Shapelet import ShapeBottleneckModel
    from utils.shapelet_project import project_
    dev = torch.device("cuda:0")
    B, C, T, K, Ls = SHAPE["B"], SHAPE["C"], SHAPE["T"], SHAPE["K"], SHAPE["L"]
    cfg = Namespace(enc_in=C, seq_len=T, num_class=3, epsilon=1.0, distance_func='euclidean', memory_efficient=False,
                    sbm_cls='linear', dropout=0.0, lambda_reg=0.1, lambda_div=0.1)
    torch.manual_seed(0)
    model = ShapeBottleneckModel(cfg, [K] * len(Ls), [L / T for L in Ls]).to(dev).eval()
    batches = [(torch.randn(B, T, C, device=dev),) for _ in range(BATCHES)]

    def forward_only():
        with torch.no_grad():
            for (x,) in batches:
                model.shapelet_features(x)

    res = dict(batches=BATCHES)
    res["forward_only_pass"] = _median_ms(forward_only)
    res["project_pass"] = _median_ms(lambda: project_(model, batches))
    res["forward_only_per_batch_ms"] = res["forward_only_pass"]["median_ms"] / BATCHES
    res["project_per_batch_ms"] = res["project_pass"]["median_ms"] / BATCHES
    res["project_over_forward"] = res["project_pass"]["median_ms"] / res["forward_only_pass"]["median_ms"]
    _lib.timing_enable(True)
    rep = project_(model, batches)
    torch.cuda.synchronize()
    ms, n = _lib.timing_read("shp_project")
    _lib.timing_enable(False)
    res["project_step_kernels"] = dict(total_ms=ms, launches=n, per_batch_ms=ms / BATCHES)
    res["kept"] = [g["kept"] for g in rep["groups"]]
    return res


STEPS = {"ordered_pass": step_pass}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shapelet_project.json"))
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
