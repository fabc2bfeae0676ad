"""Cost of the warp (not a test): one MI355X, one process, device events around windows of 20 calls after warm-up, the candidates
alternating window by window, at (B, T, C) = (256, 1651, 122) and (256, 1000, 122) with all three rates on:
  * ops.warp;
  * the torch composition of the same resampling: the source rows, weights and gains of the same map (utils.warp.warp_map) uploaded
    once as (B, T) tensors, two gathers of the batch, then the lerp and the gain -- the per-step cost of building those tensors on
    the host is NOT charged to it;
  * ops.augment (shift, gain, electrode dropout, time mask: its memory-bound form) and x.clone() as context;
  * the bytes the rule needs (one read and one write of the batch) over the time of ops.warp, as a share of the 8.0 TB/s HBM peak
    (about 6.3 TB/s is what a plain copy reaches).
The one condition: ops.warp is not slower than the torch composition at both shapes; the ratio is recorded.  The GPU work runs in a
child process under its own time limit.

    python tests/diag_warp.py [--out profiles/warp.json]        # written as the file's `diag` entry
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
WARMUP, CALLS, WINDOWS = 10, 20, 15
SHAPES = [(256, 1651, 122), (256, 1000, 122)]
HBM_PEAK = 8.0e12
RATES = dict(twarp=0.2, mwarp=0.1, wwarp=0.1)
SEED = 12345


def _windows(cands):
    """name -> sorted per-call milliseconds of WINDOWS windows of CALLS calls each, the candidates taking turns"""
    import torch
    for fn in cands.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in cands}
    for _ in range(WINDOWS):
        for name, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) / CALLS)
    return {k: sorted(v) for k, v in ts.items()}


def step_kernel():
    import numpy as np
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    from utils.warp import WarpSpec, warp_map, warp_reference
    dev = torch.device("cuda:0")
    spec = WarpSpec(**RATES)
    res = dict(hbm_peak_bytes_per_s=HBM_PEAK, calls_per_window=CALLS, windows=WINDOWS, warmup_calls=WARMUP, rates=RATES)
    for B, T, C in SHAPES:
        torch.manual_seed(0)
        x = torch.randn(B, T, C, device=dev)
        maps = [warp_map(SEED, b, T, spec) for b in range(B)]
        phi = np.stack([m[0] for m in maps])
        i0 = np.minimum(np.floor(phi).astype(np.int64), T - 2)
        idx0 = torch.from_numpy(i0).to(dev)[:, :, None].expand(B, T, C)
        idx1 = torch.from_numpy(i0 + 1).to(dev)[:, :, None].expand(B, T, C)
        w = torch.from_numpy(phi - i0.astype(np.float32)).to(dev)[:, :, None]
        g = torch.from_numpy(np.stack([m[1] for m in maps])).to(dev)[:, :, None]

        def composition():
            x0, x1 = x.gather(1, idx0), x.gather(1, idx1)
            return g * (x0 + w * (x1 - x0))
        # the two compute the same thing (the composition may fuse or reorder a rounding: 1e-6 of the data's scale, not bitwise)
        got, comp = ops.warp(x, SEED, **RATES), composition()
        err = float((got - comp).abs().max())
        assert err <= 1e-5 * float(x.abs().max()), err
        if T == 1000:
            assert np.array_equal(got[:2].cpu().numpy(), warp_reference(x[:2].cpu().numpy(), SEED, **RATES))
        ts = _windows({
            "warp": lambda: ops.warp(x, SEED, **RATES),
            "torch_composition": composition,
            "augment": lambda: ops.augment(x, SEED, shift=0.1, scale=0.1, channel_drop=0.1, time_mask=0.1),
            "clone": lambda: x.clone(),
        })
        r = {k: dict(median_ms=v[len(v) // 2], min_ms=v[0], max_ms=v[-1]) for k, v in ts.items()}
        need = 2 * x.numel() * 4
        r["bytes_needed"] = need
        r["warp_share_of_hbm_peak"] = need / (r["warp"]["median_ms"] * 1e-3) / HBM_PEAK
        r["clone_share_of_hbm_peak"] = need / (r["clone"]["median_ms"] * 1e-3) / HBM_PEAK
        r["warp_over_torch_composition"] = r["warp"]["median_ms"] / r["torch_composition"]["median_ms"]
        r["warp_over_clone"] = r["warp"]["median_ms"] / r["clone"]["median_ms"]
        r["composition_max_abs_difference"] = err
        r["warp_not_slower_than_composition"] = r["warp"]["median_ms"] <= r["torch_composition"]["median_ms"]
        res[f"{B}x{T}x{C}"] = r
        del x, idx0, idx1, w, g, got, comp
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp.json"))
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step_kernel()))
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "kernel"], capture_output=True, text=True, timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    res = json.loads(line[-1][7:]) if r.returncode == 0 and line else dict(failed=r.returncode, stderr=r.stderr[-2000:])
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}      # the file's other entries (bench) are kept
    doc["diag"] = res
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    if "failed" in res or not all(v["warp_not_slower_than_composition"] for k, v in res.items() if isinstance(v, dict) and "warp" in v):
        sys.exit(1)


if __name__ == "__main__":
    main()
