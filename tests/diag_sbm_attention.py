"""Diagnostic (not a test): the SBM attention head on its fused kernels (ops.sbm_attention) against the torch composition it
replaces, and the IGN step at the CHISCO shape with the attention head against the linear head.

    python tests/diag_sbm_attention.py --out profiles/r5_sbm_attention.json

Times are device events around `--iters` back-to-back calls after `--warmup` calls; fwd+bwd is forward plus backward.  The torch
composition (F.scaled_dot_product_attention over 16-wide q / k and a 1-wide v) runs only where its (B,F,F) intermediates are
estimated to fit in `--sdpa-gb`; elsewhere it is reported as not run, with the estimate."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import speech_imagery_eeg_amd  # noqa: E402,F401
from ign_hip import ops  # noqa: E402

SHAPES = [(256, 2440), (256, 7320), (32, 19260)]


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


def params(F_, dev):
    g = torch.Generator().manual_seed(F_)
    ps = [torch.rand(16, 1, generator=g) * 2 - 1, torch.rand(16, generator=g) * 2 - 1, torch.rand(16, 1, generator=g) * 2 - 1,
          torch.rand(16, generator=g) * 2 - 1, torch.randn(F_, 16, generator=g)]          # nn.Linear(1,16) / nn.Embedding init
    return [p.to(dev).requires_grad_() for p in ps]


def composition(x, wq, bq, wk, bk, pos):
    """models/Shapelet.py SelfAttention's torch path"""
    p = pos[:x.shape[1]]
    q = F.linear(x.unsqueeze(-1), wq, bq) + p
    k = F.linear(x.unsqueeze(-1), wk, bk) + p
    return F.scaled_dot_product_attention(q, k, x.unsqueeze(-1)).squeeze(-1)


def valu_bound_ms(B, F_):
    """The issue's VALU estimate: 8 issue units per element forward, 14 backward (v_exp_f32 = 2), wave64 FMA = 2 cycles per SIMD,
    1024 SIMDs at 2.4 GHz."""
    per_unit = 2.0 / 64 / 1024 / 2.4e9 * 1e3
    n = B * F_ * F_
    return 8 * n * per_unit, (8 + 14) * n * per_unit


def head(dev, B, F_, warmup, iters, sdpa_gb):
    x = torch.rand(B, F_, device=dev).requires_grad_()
    ps = params(F_, dev)
    gout = torch.randn(B, F_, device=dev)
    fwd_nograd = lambda: ops.sbm_attention(x.detach(), *[p.detach() for p in ps])   # noqa: E731
    fwd = lambda: ops.sbm_attention(x, *ps)                                          # noqa: E731

    def fwd_bwd():
        torch.autograd.backward(ops.sbm_attention(x, *ps), gout)

    vf, vfb = valu_bound_ms(B, F_)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    rec = dict(B=B, F=F_, fwd_nograd_ms=timed(fwd_nograd, warmup, iters), fwd_ms=timed(fwd, warmup, iters),
               fwd_bwd_ms=timed(fwd_bwd, warmup, iters), valu_bound_fwd_ms=vf, valu_bound_fwd_bwd_ms=vfb)
    rec["peak_extra_mb"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    est_gb = 4 * B * F_ * F_ * 4 / 2 ** 30          # scores, probabilities and their gradients
    rec["sdpa_estimated_gb"] = est_gb
    if est_gb > sdpa_gb:
        rec["sdpa"] = "not run: estimated intermediates above --sdpa-gb"
        return rec
    x.grad = None
    for p in ps:
        p.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    try:
        sf = timed(lambda: composition(x, *ps), warmup, iters)
        sfb = timed(lambda: torch.autograd.backward(composition(x, *ps), gout), warmup, iters)
        rec.update(sdpa_fwd_ms=sf, sdpa_fwd_bwd_ms=sfb, sdpa_peak_extra_mb=(torch.cuda.max_memory_allocated() - base) / 2 ** 20)
        with torch.no_grad():
            a, b = ops.sbm_attention(x, *ps), composition(x, *ps)
        rec["max_abs_diff_vs_sdpa"] = float((a - b).abs().max())
    except torch.cuda.OutOfMemoryError as e:                 # an allocator refusal, reported as such
        rec["sdpa"] = f"out of memory: {str(e).splitlines()[0]}"
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
    ap.add_argument("--sdpa-gb", type=float, default=100.0)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("diag_sbm_attention: needs a GPU (there is no CPU measurement)")
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), heads=[], ign_step=[])
    for B, F_ in SHAPES:
        r = head(dev, B, F_, a.warmup, a.iters, a.sdpa_gb)
        print(json.dumps(r), flush=True)
        res["heads"].append(r)
    if not a.no_step:
        for cls in ("linear", "attention", "linear", "attention"):             # alternated: the spread is visible
            r = ign_step(dev, cls, 256, a.warmup, a.iters)
            print(json.dumps(r), flush=True)
            res["ign_step"].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
