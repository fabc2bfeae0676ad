"""Cost of the artifact stage (not a test): the statistics launch (ign_eeg_artifact_stats_nct) and the apply launches
(ign_eeg_artifact_apply_nct: verdicts + tiles) at the CHISCO shape (256, 122, 1651) with clip=6,flat=0.01,noisy=8 and 3 of the 122
electrodes of every trial bad (one railed, one at 30x noise, one with a NaN), beside two yardsticks timed in the same process:
ops.eeg_iir (hp=0.5,lp=40,order=4,notch=50), the project's other one-workgroup-per-row stage, and a torch composition of the same
rule on the device -- kthvalue twice per row plus element-wise ops for the statistics, the verdicts, the clamp and the all-ones
repair.  The one condition: the stage must not be slower than the torch composition.  Device events around windows of back-to-back
calls, the candidates alternating window by window.  Bytes over HBM are counted from the shapes (statistics: one read of the batch;
apply: one read and one write) and set against the peak.  The GPU step is a child process under its own time limit.

    python tests/diag_eeg_artifact.py [--out profiles/eeg_artifact.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
WARMUP, WINDOW, ROUNDS = 5, 20, 7
SHAPE = dict(B=256, C=122, T=1651)
KEYS = dict(clip=6.0, flat=0.01, noisy=8.0)
BAD = dict(flat=17, noisy=60, nan=101)
IIR_SPEC = "hp=0.5,lp=40,order=4,notch=50"
HBM_PEAK = 8.0e12


def _windows(fns, warmup=WARMUP, window=WINDOW, rounds=ROUNDS):
    """{name: fn} -> {name: per-call ms, median over `rounds` windows of `window` calls}, the fns alternating window by window"""
    import torch
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(window):
                fn()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) / window)
    out = {}
    for name, t in ts.items():
        t.sort()
        out[name] = dict(median_ms=t[len(t) // 2], min_ms=t[0], max_ms=t[-1], windows=rounds, calls_per_window=window, warmup=warmup)
    return out


def torch_rule(x, clip, flat, noisy):
    """the rule as a torch composition on the device (all-ones weights) -> (y, verdict, stats)"""
    import torch
    B, C, T = x.shape
    k = (T - 1) // 2 + 1
    finite = torch.isfinite(x).all(-1)
    xz = torch.where(finite[..., None], x, torch.zeros((), device=x.device))
    m = xz.kthvalue(k, dim=-1).values + 0.0
    s = (xz - m[..., None]).abs().kthvalue(k, dim=-1).values
    m, s = m * finite, s * finite
    nf = finite.sum(-1)
    ref = torch.where(finite, s, torch.full((), float("inf"), device=x.device)).sort(-1).values.gather(-1, ((nf - 1).clamp(min=0) // 2)[:, None])
    ref = torch.where(nf[:, None] > 0, ref, torch.zeros((), device=x.device))
    code = torch.zeros(B, C, dtype=torch.uint8, device=x.device)
    code[s > noisy * ref] = 2
    code[s <= flat * ref] = 1
    code[~finite] = 3
    none_good = ~(code == 0).any(-1, keepdim=True)
    code = torch.where(none_good & (code != 0), torch.full((), 4, dtype=torch.uint8, device=x.device), code)
    r = (clip * 1.4826) * s
    lo, hi = (m - r)[..., None], (m + r)[..., None]
    y = torch.where(xz < lo, lo, torch.where(xz > hi, hi, xz))
    good = (code == 0)[..., None]
    mean = ((y - m[..., None]) * good).sum(1, keepdim=True) / good.sum(1, keepdim=True).clamp(min=1)
    y = torch.where(((code >= 1) & (code <= 3))[..., None], mean, y)
    return y, code, torch.stack([m, s], -1)


def step():
    import ctypes
    import numpy as np
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ops
    from utils.eeg_artifact import artifact_numpy
    from utils.eeg_iir import resolve_iir
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, C, T = SHAPE["B"], SHAPE["C"], SHAPE["T"]
    x = torch.randn(B, C, T, device=dev) * 20 + torch.empty(B, C, 1, device=dev).uniform_(-2e4, 2e4)
    x[:, BAD["flat"]] = x[:, BAD["flat"], :1]
    x[:, BAD["noisy"]] = (x[:, BAD["noisy"]] - x[:, BAD["noisy"], :1]) * 30 + x[:, BAD["noisy"], :1]
    x[:, BAD["nan"], 7] = float("nan")
    y, verdict, stats = ops.eeg_artifact(x, **KEYS)
    flags = (verdict == 3).to(torch.uint8) * 3
    L, p, s = _lib.lib(), (lambda t: ctypes.c_void_p(t.data_ptr())), _lib.stream
    y2, v2, s2 = torch.empty_like(y), torch.empty_like(verdict), torch.empty_like(stats)
    f2 = torch.empty_like(flags)
    iir = resolve_iir(IIR_SPEC, T)
    coef, yi = torch.from_numpy(iir.table).to(dev), torch.empty_like(x)
    xi = torch.nan_to_num(x)
    fns = {
        "stats": lambda: _lib.check(L.ign_eeg_artifact_stats_nct(p(x), p(s2), p(f2), B, C, T, s()), "stats"),
        "apply": lambda: _lib.check(L.ign_eeg_artifact_apply_nct(p(x), p(stats), p(flags), None, p(y2), p(v2), B, C, T, KEYS["clip"],
                                                                 KEYS["flat"], KEYS["noisy"], s()), "apply"),
        "stage": lambda: ops.eeg_artifact(x, out=(y2, v2, s2), **KEYS),
        "yardstick_eeg_iir": lambda: ops.eeg_iir(xi, coef, pad=iir.pad, g0=iir.g0, out=yi),
        "yardstick_torch_composition": lambda: torch_rule(x, **KEYS),
    }
    res = dict(hbm_peak_bytes_per_s=HBM_PEAK, shape=SHAPE, keys=KEYS, bad_electrodes_per_trial=3, iir_spec=IIR_SPEC)
    res.update(_windows(fns))
    nbytes = dict(stats=4 * B * C * T, apply=8 * B * C * T, stage=12 * B * C * T)
    for name, nb in nbytes.items():
        res[name].update(bytes=nb, share_of_hbm_peak=nb / (res[name]["median_ms"] * 1e-3) / HBM_PEAK)
    res["lds_bytes_per_row_when_staged"] = int(L.ign_eeg_artifact_lds_bytes(T))
    res["lds_bytes_per_row"] = 0 if T <= 2048 else res["lds_bytes_per_row_when_staged"]      # up to 2048 samples: registers, one wave per row
    res["verdict_counts"] = {str(c): int((verdict == c).sum()) for c in range(5)}
    again = ops.eeg_artifact(x, **KEYS)
    res["two_calls_bitwise"] = bool(all(torch.equal(a, b) for a, b in zip(again, (y, verdict, stats))))
    ty, tv, ts = torch_rule(x, **KEYS)
    res["torch_composition_same_verdicts_and_stats"] = bool(torch.equal(tv, verdict) and torch.equal(ts, stats))
    want = artifact_numpy(x[:2].cpu().numpy(), **KEYS)                  # two trials against the numpy rule
    res["two_trials_stats_and_verdicts_exact"] = bool(np.array_equal(want[1], verdict[:2].cpu().numpy())
                                                      and np.array_equal(want[2], stats[:2].cpu().numpy()))
    res["stage_over_torch_composition"] = res["stage"]["median_ms"] / res["yardstick_torch_composition"]["median_ms"]
    res["stage_over_eeg_iir"] = res["stage"]["median_ms"] / res["yardstick_eeg_iir"]["median_ms"]
    res["stats_over_eeg_iir"] = res["stats"]["median_ms"] / res["yardstick_eeg_iir"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eeg_artifact.json"))
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step()))
        return
    limit = 300
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step"], capture_output=True, text=True, timeout=limit)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        rc, err = r.returncode, r.stderr[-2000:]
    except subprocess.TimeoutExpired:
        line, rc, err = [], 124, f"no result within {limit} s"
    if rc != 0 or not line:
        res = dict(failed=rc, stderr=err)
        print("failed", rc, err, flush=True)
    else:
        res = json.loads(line[-1][7:])
        print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    if "failed" in res:
        sys.exit(1)


if __name__ == "__main__":
    main()
