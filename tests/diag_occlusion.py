"""Timing of the occlusion passes (not a test) at (B, T, C) = (32, 1000, 122), window=50, stride=25, groups="all" (P = 39 patches),
rows=256 (8 patches per launch): ign_occlude_btc against a copy_ of the same output bytes (its floor: one read per 8 writes) and
against the torch composition of the same result (repeat_interleave plus a masked where); ign_occlusion_spread against a clone of the
map; and the share of an occlusion_map call on the benchmark's InterpGN(FCN) model that is spent outside the model forwards.
Warm-up, then the median of repeated event-timed runs; every leg is a child process under its own time limit, and nothing more is
started after one fails.

    python tests/diag_occlusion.py [--out profiles/occlusion.json]
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
B, T, C, WINDOW, STRIDE, ROWS = 32, 1000, 122, 50, 25, 256


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


def leg_kernels():
    import numpy as np
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    from utils.occlusion import grid
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, T, C, device=dev, generator=g)
    fill = x.mean(1).contiguous()
    W, S, nt = grid(T, WINDOW, STRIDE)
    gid, G, Pc = np.zeros(C, np.int32), 1, ROWS // B
    drop = torch.randn(B, nt * G, device=dev, generator=g)
    out = ops.occlude(x, 8, Pc, gid, G, WINDOW, STRIDE, fill=fill)
    src = torch.randn_like(out)
    lo = (torch.arange(8, 8 + Pc, device=dev) * S)[None, :, None, None]
    t = torch.arange(T, device=dev)[None, None, :, None]

    def composed():
        rep = x.repeat_interleave(Pc, dim=0).view(B, Pc, T, C)
        return torch.where((t >= lo) & (t < lo + W), fill[:, None, None, :], rep).view(B * Pc, T, C)

    assert torch.equal(composed().view(torch.int32), out.view(torch.int32))                # the same result, bit for bit
    occ = _median_ms(lambda: ops.occlude(x, 8, Pc, gid, G, WINDOW, STRIDE, fill=fill))
    copy = _median_ms(lambda: out.copy_(src))
    comp = _median_ms(composed)
    m = ops.occlusion_spread(drop, gid, G, WINDOW, STRIDE, T)
    spread = _median_ms(lambda: ops.occlusion_spread(drop, gid, G, WINDOW, STRIDE, T))
    clone = _median_ms(lambda: m.clone())
    return dict(occlude=occ, copy_same_bytes=copy, torch_composition=comp, spread=spread, clone_map=clone,
                occlude_over_copy=occ["median_ms"] / copy["median_ms"], occlude_over_torch=occ["median_ms"] / comp["median_ms"],
                spread_over_clone=spread["median_ms"] / clone["median_ms"],
                occlude_GB_per_s=(Pc + 1) * x.numel() * 4 / occ["median_ms"] / 1e6)


def leg_model():
    """occlusion_map on the benchmark's model, timed whole (host clock around a synchronise) and with the forwards alone"""
    import time
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from bench import ch_config
    from models.InterpGN import InterpGN
    from utils import occlusion as O
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = InterpGN(ch_config()).to(dev).eval()
    x = torch.randn(B, T, C, device=dev)
    W, S, nt = O.grid(T, WINDOW, STRIDE)
    Pc = ROWS // B
    sizes = [min(Pc, nt - p0) for p0 in range(0, nt, Pc)]
    copies = {n: torch.randn(B * n, T, C, device=dev) for n in set(sizes)}

    def whole():
        O.occlusion_map(model, x, explain="model", window=WINDOW, stride=STRIDE, groups="all", rows=ROWS)

    def forwards():
        with torch.no_grad():
            model(x, None, None, None)
            for n in sizes:
                model(copies[n], None, None, None)

    def wall(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(9):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return dict(median_ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1], runs=9, warmup=3)

    a, b, a2 = wall(whole), wall(forwards), wall(whole)
    med = 0.5 * (a["median_ms"] + a2["median_ms"])
    return dict(occlusion_map=a, occlusion_map_again=a2, forwards_alone=b, patches=nt, forwards=1 + len(sizes),
                share_outside_forwards=1.0 - b["median_ms"] / med)


LEGS = {"kernels": leg_kernels, "model": leg_model}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occlusion.json"))
    a = ap.parse_args()
    if a.leg:
        print("RESULT " + json.dumps(LEGS[a.leg]()))
        return
    res = dict(shape=dict(B=B, T=T, C=C, window=WINDOW, stride=STRIDE, groups="all", rows=ROWS))
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
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
