"""Timing of the faithfulness passes (not a test) at the CHISCO shape (B, T, C) = (256, 1651, 122), a score per cell, steps = 10:
ign_rank_threshold (all 11 thresholds in one launch) and one ign_perturb_btc, against the torch composition of the same result --
torch.sort of the (B, T*C) scores, descending and stable, then a scatter mask and torch.where -- and against a clone of the batch.
Warm-up, then the median of repeated event-timed runs; every leg is a child process under its own time limit, and nothing more is
started after one fails.

    python tests/diag_faithfulness.py [--out profiles/faithfulness.json]
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
B, T, C, STEPS = 256, 1651, 122, 10


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


def _inputs(kind):
    """x, the score map and the k table.  "random": distinct scores; "windows": an evidence-like map, zero but for constant windows"""
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, T, C, device=dev, generator=g)
    if kind == "random":
        score = torch.rand(B, T, C, device=dev, generator=g)
    else:
        score = torch.zeros(B, T, C, device=dev)
        for i in range(20):
            t0 = 70 * i + 11
            score[:, t0:t0 + 100 + 20 * i, (7 * i) % C] += 0.125 * (i + 1)
    n = T * C
    k = torch.tensor([[(j * n) // STEPS for j in range(STEPS + 1)]] * B, dtype=torch.int32, device=dev)
    return x, score, k


def leg_hip(kind):
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    x, score, k = _inputs(kind)
    fill = x.mean(1).contiguous()
    key, idx = ops.rank_threshold(score, k)
    rank = _median_ms(lambda: ops.rank_threshold(score, k))
    perturb = _median_ms(lambda: ops.perturb(x, score, key, idx, STEPS // 2, fill=fill))
    clone = _median_ms(lambda: x.clone())
    return dict(rank_threshold=rank, perturb=perturb, clone=clone, pair_ms=rank["median_ms"] + perturb["median_ms"],
                curve_ms=rank["median_ms"] + (STEPS + 1) * perturb["median_ms"],
                perturb_over_clone=perturb["median_ms"] / clone["median_ms"],
                perturb_GB_per_s=3 * x.numel() * 4 / perturb["median_ms"] / 1e6)


def leg_torch(kind):
    import torch
    x, score, k = _inputs(kind)
    fill = x.mean(1).contiguous()
    n = T * C
    kk = (STEPS // 2 * n) // STEPS

    def sort():
        return torch.sort(score.view(B, n), dim=1, descending=True, stable=True).indices

    order = sort()

    def apply():
        mask = torch.zeros(B, n, dtype=torch.bool, device=x.device)
        mask.scatter_(1, order[:, :kk], True)
        return torch.where(mask.view(B, T, C), fill[:, None, :], x)

    s, a = _median_ms(sort), _median_ms(apply)
    return dict(sort=s, scatter_where=a, pair_ms=s["median_ms"] + a["median_ms"],
                curve_ms=s["median_ms"] + (STEPS + 1) * a["median_ms"], index_bytes=order.numel() * order.element_size())


LEGS = {"hip_random": lambda: leg_hip("random"), "torch_random": lambda: leg_torch("random"),
        "hip_windows": lambda: leg_hip("windows"), "torch_windows": lambda: leg_torch("windows")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "faithfulness.json"))
    a = ap.parse_args()
    if a.leg:
        print("RESULT " + json.dumps(LEGS[a.leg]()))
        return
    res = dict(shape=dict(B=B, T=T, C=C, Cs=C, steps=STEPS))
    ok = True
    for name in LEGS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name], capture_output=True, text=True, timeout=240)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            res[name] = dict(failed=r.returncode, stderr=r.stderr[-2000:])
            ok = False
            break                                   # nothing more is started on the GPU after a failed leg
        res[name] = json.loads(line[-1][7:])
        print(name, json.dumps(res[name]), flush=True)
    if ok:
        for kind in ("random", "windows"):
            res[f"pair_hip_over_torch_{kind}"] = res[f"hip_{kind}"]["pair_ms"] / res[f"torch_{kind}"]["pair_ms"]
            res[f"curve_hip_over_torch_{kind}"] = res[f"hip_{kind}"]["curve_ms"] / res[f"torch_{kind}"]["curve_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
