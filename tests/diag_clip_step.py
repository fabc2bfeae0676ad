"""Diagnostic: what gradient clipping costs one IGN(FCN) training step -- kernel launches and ms per step -- at the benchmark shape
(C 122, T 1000, 3 classes, B 256) and at BasicMotions (C 6, T 100, 4 classes, B 32), for

  unclipped    forward, fused loss, backward, FlatAdam.step()                                   (the launch-count baseline)
  torch_clip   ... nn.utils.clip_grad_norm_ on the flat-buffer views, then FlatAdam.step()      (the step before ign_grad_norm_clip)
  hip_clip     ... FlatAdam.step(max_norm=0.5): one ign_grad_norm_clip launch, coefficient folded into Adam
  hip_clip_graph   the same step captured into a hipGraph and replayed (capturable FlatAdam)

    python tests/diag_clip_step.py [--out profiles/clip_step.json]

Every (shape, configuration) runs in a child process of its own under its own time limit; the first child that fails or runs out of
time ends the run (nothing more is started on the GPU) and no file is written."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"bench": dict(C=122, T=1000, NC=3, B=256), "bm32": dict(C=6, T=100, NC=4, B=32)}
CONFIGS = ("unclipped", "torch_clip", "hip_clip", "hip_clip_graph")
CHILD_LIMIT_S = 240
MAX_NORM = 0.5


def child(shape, config, steps, warmup):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from conftest import make_cfg
    from ign_hip import ops as ign_ops
    from ign_hip.ddp import FlatAdam, FlatParamBucket
    from ign_hip.graph import GraphedTrainStep
    from models.InterpGN import InterpGN
    from torch.profiler import ProfilerActivity, profile

    s = SHAPES[shape]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = InterpGN(make_cfg(enc_in=s["C"], seq_len=s["T"], num_class=s["NC"])).to(dev).train()
    bucket = FlatParamBucket(model, 1)
    graph = config == "hip_clip_graph"
    opt = FlatAdam(bucket, lr=5e-3, capturable=graph)
    x = torch.randn(s["B"], s["T"], s["C"], device=dev)
    y = torch.randint(0, s["NC"], (s["B"],), device=dev)
    mask = torch.ones(s["B"], s["T"], device=dev)

    def step(x, y):
        _, info = model(x, mask, None, None)
        loss = ign_ops.ign_loss(info.shapelet_preds, info.dnn_preds, y, 1.0, reg=info.loss)[0]
        ign_ops.backward(loss)
        if config == "torch_clip":
            bucket.gather()
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=MAX_NORM)
        opt.step(max_norm=MAX_NORM if config.startswith("hip_clip") else None)
        bucket.zero_grad()
        return loss.detach()

    run = GraphedTrainStep(step, (x, y), warmup=3) if graph else step
    for _ in range(warmup):
        run(x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run(x, y)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(2):
            run(x, y)
        torch.cuda.synchronize()
    launches = sum(1 for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA")
                   and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower()) / 2
    norm = None if opt.last_grad_norm is None else float(opt.last_grad_norm)
    print("RESULT " + json.dumps({"shape": shape, "config": config, "ms_per_step": round(ms, 4), "launches_per_step": launches,
                                  "steps": steps, "grad_norm": norm, "flat_floats": bucket.flat_grad.numel()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_step.json"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "CONFIG"))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.steps, a.warmup)
    rows = []
    for shape in SHAPES:
        for config in CONFIGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, config, "--steps", str(a.steps), "--warmup",
                   str(a.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
            except subprocess.TimeoutExpired:
                sys.exit(f"{shape}/{config}: no result within {CHILD_LIMIT_S} s; stopping")
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.exit(f"{shape}/{config}: exit status {r.returncode}; stopping\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
            rows.append(json.loads(line[-1][len("RESULT "):]))
            print(rows[-1], flush=True)
    out = {"what": "IGN(FCN) training step, fp32, one GPU: clipping at max_norm 0.5 (tests/diag_clip_step.py)", "rows": rows,
           "ratios": {}}
    for shape in SHAPES:
        by = {r["config"]: r for r in rows if r["shape"] == shape}
        out["ratios"][shape] = {
            "hip_clip_ms_over_torch_clip_ms": round(by["hip_clip"]["ms_per_step"] / by["torch_clip"]["ms_per_step"], 4),
            "hip_clip_graph_ms_over_torch_clip_ms": round(by["hip_clip_graph"]["ms_per_step"] / by["torch_clip"]["ms_per_step"], 4),
            "hip_clip_launches_minus_unclipped": by["hip_clip"]["launches_per_step"] - by["unclipped"]["launches_per_step"],
            "torch_clip_launches_minus_unclipped": by["torch_clip"]["launches_per_step"] - by["unclipped"]["launches_per_step"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
