"""Cost of the evidence maps (not a test): one MI355X, one process, device events around windows of 20 calls after warm-up, the
candidates alternating window by window.
  * ops.shapelet_evidence at (B, T, C) = (256, 1000, 122) and (256, 1651, 122), with the default bank (4 groups x 5 shapelets of
    10 / 20 / 30 / 50 % of T) and the 6 x 10 bank, against
      - the torch composition of the same map: per group the (B, K, C) values scattered with both signs into a (B, T + 1, C)
        difference array at the window's two ends, summed over the groups, then one cumsum along time;
      - x.clone() of a (B, T, C) tensor as the write-bound floor;
    and the one (B, T, C) write the rule needs over the kernel's time, as a share of the 8.0 TB/s HBM peak.
  * ops.fcn_cam + ops.cam_spread at (256, 987, 128) (block 3's output at T = 1000) against torch.relu(y * a + b) contracted with
    Wfc[target], then a box filter; the one read of y_last over the two launches' time as a share of the HBM peak.
The one condition: neither is slower than its torch composition at any shape; the ratios are recorded.  The GPU work runs in a child
process under its own time limit.

    python tests/diag_evidence.py [--out profiles/evidence.json]        # written as the file's `diag` entry
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
SHAPES = [(256, 1000, 122), (256, 1651, 122)]
BANKS = {"4x5": ([5] * 4, [0.1, 0.2, 0.3, 0.5]), "6x10": ([10] * 6, [0.05, 0.1, 0.2, 0.3, 0.4, 0.5])}
CAM_SHAPE = (256, 987, 128)
N_CLASS = 39
HBM_PEAK = 8.0e12


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


def _kernel_only(labels, fn):
    """milliseconds per call of the library's own launches under `labels` (ign_timing_*: events around each launch), without the
    host side of the op"""
    import torch
    from ign_hip import _lib
    torch.cuda.synchronize()
    _lib.timing_enable(True)
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    ms = sum(_lib.timing_read(lb)[0] for lb in labels) / CALLS
    _lib.timing_enable(False)
    return ms


def _stats(ts):
    return {k: dict(median_ms=v[len(v) // 2], min_ms=v[0], max_ms=v[-1]) for k, v in ts.items()}


def step_kernel():
    import math
    import torch
    import torch.nn.functional as F
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    dev = torch.device("cuda:0")
    res = dict(hbm_peak_bytes_per_s=HBM_PEAK, calls_per_window=CALLS, windows=WINDOWS, warmup_calls=WARMUP, classes=N_CLASS)
    for B, T, C in SHAPES:
        for bank, (Ks, fracs) in BANKS.items():
            torch.manual_seed(0)
            Ls = [max(3, math.ceil(f * T)) for f in fracs]
            strides = [1] * len(Ks)
            ld = sum(Ks) * C
            p = torch.rand(B, ld, device=dev)
            W = torch.randn(N_CLASS, ld, device=dev)
            target = torch.randint(0, N_CLASS, (B,), device=dev)
            t = torch.cat([torch.randint(0, T - L + 1, (B, K * C), device=dev) for K, L in zip(Ks, Ls)], 1).to(torch.int32)
            x = torch.randn(B, T, C, device=dev)
            tl = t.long()

            def composition():
                v = W[target] * p
                diff = torch.zeros(B, T + 1, C, device=dev)
                col0 = 0
                for K, L in zip(Ks, Ls):
                    vg = (v[:, col0:col0 + K * C] / L).view(B, K, C)
                    st = tl[:, col0:col0 + K * C].view(B, K, C)
                    diff.scatter_add_(1, st, vg)
                    diff.scatter_add_(1, st + L, -vg)
                    col0 += K * C
                return diff.cumsum(1)[:, :T]

            got, comp = ops.shapelet_evidence(p, t, W, target, Ks, Ls, strides, C, T), composition()
            err = float((got - comp).abs().max())
            assert err <= 1e-3 * float(got.abs().max()), err           # (a running sum over T steps against a sum of <= sum K terms)
            r = _stats(_windows({
                "shapelet_evidence": lambda: ops.shapelet_evidence(p, t, W, target, Ks, Ls, strides, C, T),
                "torch_composition": composition,
                "clone": lambda: x.clone(),
            }))
            need = x.numel() * 4
            k, c, cl = (r[n]["median_ms"] for n in ("shapelet_evidence", "torch_composition", "clone"))
            ko = _kernel_only(["evidence"], lambda: ops.shapelet_evidence(p, t, W, target, Ks, Ls, strides, C, T))
            r.update(kernel_only_ms=ko, kernel_only_share_of_hbm_peak=need / (ko * 1e-3) / HBM_PEAK, kernel_only_over_clone=ko / cl)
            r.update(bytes_needed=need, kernel_share_of_hbm_peak=need / (k * 1e-3) / HBM_PEAK, kernel_over_torch_composition=k / c,
                     kernel_over_clone=k / cl, composition_max_abs_difference=err, kernel_not_slower_than_composition=k <= c,
                     Ks=Ks, Ls=Ls)
            res[f"evidence {B}x{T}x{C} bank {bank}"] = r
            del p, W, t, tl, x, got, comp
            torch.cuda.empty_cache()
    B, Tl, Cl = CAM_SHAPE
    R = 14
    torch.manual_seed(1)
    y = torch.randn(B, Tl, Cl, device=dev)
    a, b = torch.rand(Cl, device=dev) + 0.5, torch.randn(Cl, device=dev) * 0.3
    Wfc = torch.randn(N_CLASS, Cl, device=dev)
    target = torch.randint(0, N_CLASS, (B,), device=dev)
    box = torch.full((1, 1, R), 1.0 / R, device=dev)

    def cam_composition():
        cam = torch.bmm(torch.relu(y * a + b), Wfc[target][:, :, None]).squeeze(-1) / Tl
        return cam, F.conv1d(cam[:, None, :], box, padding=R - 1)[:, 0]

    def cam_kernels():
        cam = ops.fcn_cam(y, a, b, Wfc, target)
        return cam, ops.cam_spread(cam, R)

    (cam, dnn), (cam_c, dnn_c) = cam_kernels(), cam_composition()
    errs = float((cam - cam_c).abs().max()), float((dnn - dnn_c).abs().max())
    assert errs[0] <= 1e-4 * float(cam.abs().max()) and errs[1] <= 1e-4 * float(dnn.abs().max()), errs
    r = _stats(_windows({"fcn_cam_and_spread": cam_kernels, "fcn_cam": lambda: ops.fcn_cam(y, a, b, Wfc, target),
                         "torch_composition": cam_composition, "clone": lambda: y.clone()}))
    need = y.numel() * 4
    k, c = r["fcn_cam_and_spread"]["median_ms"], r["torch_composition"]["median_ms"]
    ko = _kernel_only(["bn_relu_cam"], lambda: ops.fcn_cam(y, a, b, Wfc, target))
    r.update(cam_kernel_only_ms=ko, cam_kernel_only_share_of_hbm_peak=need / (ko * 1e-3) / HBM_PEAK)
    r.update(bytes_needed=need, kernels_share_of_hbm_peak=need / (k * 1e-3) / HBM_PEAK,
             cam_alone_share_of_hbm_peak=need / (r["fcn_cam"]["median_ms"] * 1e-3) / HBM_PEAK, kernels_over_torch_composition=k / c,
             composition_max_abs_difference=list(errs), kernel_not_slower_than_composition=k <= c)
    res[f"cam {B}x{Tl}x{Cl}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evidence.json"))
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step_kernel()))
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "kernel"], capture_output=True, text=True, timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    res = json.loads(line[-1][7:]) if r.returncode == 0 and line else dict(failed=r.returncode, stderr=r.stderr[-2000:])
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}      # the file's other entries (bench, resources) are kept
    doc["diag"] = res
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    if "failed" in res or not all(v["kernel_not_slower_than_composition"] for v in res.values()
                                  if isinstance(v, dict) and "kernel_not_slower_than_composition" in v):
        sys.exit(1)


if __name__ == "__main__":
    main()
