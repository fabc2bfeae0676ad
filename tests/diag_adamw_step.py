"""Diagnostic: what AdamW with a per-step cosine schedule, and the EMA of the weights, cost one IGN(FCN) training step -- kernel
launches and ms per step -- at the benchmark shape (C 122, T 1000, 3 classes, B 256) and at BasicMotions (C 6, T 100, 4 classes,
B 32), for

  adam                    forward, fused loss, backward, FlatAdam.step() in host-count form           (today's path)
  adam_again              the same a second time                                                        (the run-to-run spread)
  adamw_cosine            FlatAdam(weight_decay=0.01, schedule="cosine,warmup=10"): tick + ign_adamw_step_dev
  adamw_cosine_ema        ... and FlatAdam.ema_update() after the step (ema 0.999)
  adamw_cosine_graph      adamw_cosine captured into a hipGraph and replayed
  adamw_cosine_ema_graph  adamw_cosine_ema captured into a hipGraph and replayed

    python tests/diag_adamw_step.py [--out profiles/adamw_step.json]

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
CONFIGS = ("adam", "adam_again", "adamw_cosine", "adamw_cosine_ema", "adamw_cosine_graph", "adamw_cosine_ema_graph")
CHILD_LIMIT_S = 240


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
    graph, ema = config.endswith("_graph"), "_ema" in config
    if config.startswith("adamw"):
        opt = FlatAdam(bucket, lr=5e-3, weight_decay=0.01, schedule="cosine,warmup=10", total_steps=steps + warmup + 8,
                       ema=0.999 if ema else 0.0)
    else:
        opt = FlatAdam(bucket, lr=5e-3)
    x = torch.randn(s["B"], s["T"], s["C"], device=dev)
    y = torch.randint(0, s["NC"], (s["B"],), device=dev)
    mask = torch.ones(s["B"], s["T"], device=dev)

    def step(x, y):
        _, info = model(x, mask, None, None)
        loss = ign_ops.ign_loss(info.shapelet_preds, info.dnn_preds, y, 1.0, reg=info.loss)[0]
        ign_ops.backward(loss)
        opt.step()
        if ema:
            opt.ema_update()
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
    print("RESULT " + json.dumps({"shape": shape, "config": config, "ms_per_step": round(ms, 4), "launches_per_step": launches,
                                  "steps": steps, "flat_floats": bucket.flat_grad.numel()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_step.json"))
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
    out = {"what": "IGN(FCN) training step, fp32, one GPU: Adam against AdamW + cosine schedule (+ EMA) (tests/diag_adamw_step.py)",
           "rows": rows, "ratios": {}}
    for shape in SHAPES:
        by = {r["config"]: r for r in rows if r["shape"] == shape}
        adam = by["adam"]["ms_per_step"]
        out["ratios"][shape] = {
            "adam_again_ms_over_adam_ms": round(by["adam_again"]["ms_per_step"] / adam, 4),
            "adamw_cosine_ms_over_adam_ms": round(by["adamw_cosine"]["ms_per_step"] / adam, 4),
            "adamw_cosine_ema_ms_over_adam_ms": round(by["adamw_cosine_ema"]["ms_per_step"] / adam, 4),
            "adamw_cosine_launches_minus_adam": by["adamw_cosine"]["launches_per_step"] - by["adam"]["launches_per_step"],
            "adamw_cosine_ema_launches_minus_adamw_cosine": by["adamw_cosine_ema"]["launches_per_step"]
            - by["adamw_cosine"]["launches_per_step"],
            "ema_graph_ms_over_graph_ms": round(by["adamw_cosine_ema_graph"]["ms_per_step"] / by["adamw_cosine_graph"]["ms_per_step"], 4)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
