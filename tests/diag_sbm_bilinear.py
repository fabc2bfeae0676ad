"""Diagnostic (not a test): the SBM bilinear head on its fp32 matrix-core kernels (ops.sbm_bilinear) against the nn.Bilinear
composition it replaces, each kernel's share of the fp32 matrix peak, and the IGN step at the CHISCO shape with the bilinear
head against the linear head.

    python tests/diag_sbm_bilinear.py --out profiles/r6_sbm_bilinear.json

Times are device events around `--iters` back-to-back calls after `--warmup` calls; fwd+bwd is forward plus backward.  The
kernel split calls the C ABI directly: the forward (GEMM + row dot, then the tile-order sum), the backward with only gu (the dU
GEMMs, then the class-order sum), with only gv (the elementwise dV), and with only gw (the dW GEMM).  nn.Bilinear runs only
where its (B,F,F) backward temporary is estimated to fit in `--torch-gb`; elsewhere it is reported as not run, with the
estimate."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import speech_imagery_eeg_amd  # noqa: E402,F401
from ign_hip import _lib, ops  # noqa: E402

SHAPES = [(256, 2440, 3), (256, 7320, 3), (32, 360, 4)]
F32_MATRIX_PEAK = 157.3e12          # FLOP/s, v_mfma_f32_32x32x2_f32 on all 256 CUs


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def share(flop, ms):
    return flop / (ms * 1e-3) / F32_MATRIX_PEAK


def kernels(u, v, w, gout, warmup, iters):
    """per-kernel times and peak shares through the C ABI"""
    B, F_ = u.shape
    N = w.shape[0]
    L, p, s = _lib.lib(), ops._ptr, _lib.stream
    out = torch.empty(B, N, device=u.device)
    t = torch.empty(B, N, F_, device=u.device)
    ws = torch.empty(L.ign_sbm_bilinear_workspace_bytes(B, F_, N) // 4, device=u.device)     # forward and backward in turn
    gu, gv, gw = torch.empty_like(u), torch.empty_like(v), torch.empty_like(w)
    gemm = 2.0 * B * N * F_ * F_

    def fwd():
        _lib.check(L.ign_sbm_bilinear_fwd(p(u), p(v), p(w), p(out), p(t), p(ws), B, F_, N, s()), "fwd")

    def bwd(a, b, c):
        return lambda: _lib.check(L.ign_sbm_bilinear_bwd(p(u), p(v), p(w), p(t), p(gout), p(a), p(b), p(c), p(ws), B, F_, N, s()),
                                  "bwd")

    rec = dict(fwd_ms=timed(fwd, warmup, iters), dgrad_gu_ms=timed(bwd(gu, None, None), warmup, iters),
               dgrad_gv_ms=timed(bwd(None, gv, None), warmup, iters), wgrad_ms=timed(bwd(None, None, gw), warmup, iters))
    rec["fwd_peak_share"] = share(gemm, rec["fwd_ms"])
    rec["dgrad_gu_peak_share"] = share(gemm, rec["dgrad_gu_ms"])
    rec["wgrad_peak_share"] = share(gemm, rec["wgrad_ms"])
    three = rec["fwd_ms"] + rec["dgrad_gu_ms"] + rec["wgrad_ms"]
    rec["three_gemms_ms"] = three
    rec["three_gemms_peak_share"] = share(3 * gemm, three)
    return rec


def head(dev, B, F_, N, warmup, iters, torch_gb, with_torch=True):
    g = torch.Generator().manual_seed(F_)
    u = torch.rand(B, F_, generator=g).to(dev).requires_grad_()
    v = torch.rand(B, F_, generator=g).to(dev).requires_grad_()
    w = ((torch.rand(N, F_, F_, generator=g) * 2 - 1) / F_ ** 0.5).to(dev).requires_grad_()
    gout = torch.randn(B, N, generator=g).to(dev)
    fwd_nograd = lambda: ops.sbm_bilinear(u.detach(), v.detach(), w.detach())   # noqa: E731

    def fwd_bwd():
        torch.autograd.backward(ops.sbm_bilinear(u, v, w), gout)

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    rec = dict(B=B, F=F_, N=N, fwd_nograd_ms=timed(fwd_nograd, warmup, iters), fwd_bwd_ms=timed(fwd_bwd, warmup, iters))
    rec["peak_extra_mb"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    gemm = 2.0 * B * N * F_ * F_
    rec["gemm_gflop_each"] = gemm / 1e9
    rec["fwd_bwd_peak_share"] = share(3 * gemm, rec["fwd_bwd_ms"])
    rec["kernels"] = kernels(u.detach(), v.detach(), w.detach(), gout, warmup, iters)
    est_gb = B * F_ * F_ * 4 / 1e9                  # nn.Bilinear's backward: one (B,F,F) fp32 temporary per class
    rec["torch_temporary_gb_per_class"] = est_gb
    if not with_torch:
        return rec
    if est_gb > torch_gb:
        rec["torch"] = f"not run: (B,F,F) temporary of {est_gb:.1f} GB per class above --torch-gb {torch_gb}"
        return rec
    u.grad = v.grad = w.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    try:
        tf = timed(lambda: F.bilinear(u.detach(), v.detach(), w.detach()), warmup, iters)
        tfb = timed(lambda: torch.autograd.backward(F.bilinear(u, v, w), gout), warmup, iters)
        rec.update(torch_fwd_ms=tf, torch_fwd_bwd_ms=tfb, torch_peak_extra_mb=(torch.cuda.max_memory_allocated() - base) / 2 ** 20)
        with torch.no_grad():
            a, b = ops.sbm_bilinear(u, v, w), F.bilinear(u, v, w)
        rec["max_abs_diff_vs_torch"] = float((a - b).abs().max())
        rec["fwd_bwd_speedup_vs_torch"] = tfb / rec["fwd_bwd_ms"]
    except torch.cuda.OutOfMemoryError as e:                 # an allocator refusal, reported as such
        rec["torch"] = f"out of memory: {str(e).splitlines()[0]}"
    return rec


def ign_step(dev, sbm_cls, B, warmup, iters):
    from bench import ch_config
    from ign_hip.ddp import FlatAdam, FlatParamBucket
    from models.InterpGN import InterpGN
    cfg = ch_config()
    cfg.sbm_cls = sbm_cls
    torch.manual_seed(0)
    model = InterpGN(cfg).to(dev).train()
    bucket = FlatParamBucket(model, 1)
    opt = FlatAdam(bucket, lr=5e-3)
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(B, cfg.seq_len, cfg.enc_in, generator=g).to(dev)
    y = torch.randint(0, cfg.num_class, (B,), generator=g).to(dev)
    mask = torch.ones(B, cfg.seq_len, device=dev)

    def step():
        out, info = model(x, mask, None, None)
        loss = ops.ign_loss(info.shapelet_preds, info.dnn_preds, y, 1.0, reg=info.loss)[0]
        ops.backward(loss)
        opt.step()
        bucket.zero_grad()

    return dict(sbm_cls=sbm_cls, B=B, features=model.sbm.total_shapelets, step_ms=timed(step, warmup, iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-gb", type=float, default=40.0)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="the kernel path at (256, 2440, 3) only (for a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("diag_sbm_bilinear: needs a GPU (there is no CPU measurement)")
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), f32_matrix_peak_tflops=F32_MATRIX_PEAK / 1e12, heads=[], ign_step=[])
    for B, F_, N in SHAPES[:1] if a.kernels_only else SHAPES:
        r = head(dev, B, F_, N, a.warmup, a.iters, a.torch_gb, with_torch=not a.kernels_only)
        print(json.dumps(r), flush=True)
        res["heads"].append(r)
    if not a.no_step and not a.kernels_only:
        for cls in ("linear", "bilinear", "linear", "bilinear"):             # alternated: the spread is visible
            r = ign_step(dev, cls, 256, a.warmup, a.iters)
            print(json.dumps(r), flush=True)
            res["ign_step"].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
