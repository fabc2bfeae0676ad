"""Cost of a wide class head: the IGN(FCN) training step at the CHISCO shape (B 256, C 122, T 1000) with 3 and with 39 classes,
and the head / loss kernels on their own at the same shapes.  A measuring script, not a test.

    python tests/diag_many_class.py [--steps 20] [--json results.json]
For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python tests/diag_many_class.py`.
Prints one line per class count; `--json` also writes them to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def _time(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(steps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def step_ms(N, steps):
    import speech_imagery_eeg_amd  # noqa: F401
    from conftest import make_cfg
    from ign_hip import ops
    from ign_hip.ddp import FlatAdam, FlatParamBucket
    from models.InterpGN import InterpGN
    dev = torch.device("cuda:0")
    cfg = make_cfg(enc_in=122, seq_len=1000, num_class=N, c_out=N)
    torch.manual_seed(0)
    model = InterpGN(cfg).to(dev).train()
    bucket = FlatParamBucket(model, 1)
    opt = FlatAdam(bucket, lr=5e-3)
    x = torch.randn(256, 1000, 122, device=dev)
    y = (torch.arange(256) % N).to(dev)

    def step():
        out, info = model(x, None, None, None)
        loss = ops.ign_loss(info.shapelet_preds, info.dnn_preds, y, 1.0, reg=info.loss)[0]
        ops.backward(loss)
        opt.step()
        bucket.zero_grad()

    return _time(step, steps)


def kernels_ms(N, steps, B=256, F_=2440):
    import ctypes
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    dev = torch.device("cuda:0")
    X, W = torch.randn(B, F_, device=dev), torch.randn(N, F_, device=dev)
    g, out = torch.randn(B, N, device=dev), torch.empty(B, N, device=dev)
    gX, gW = torch.empty(B, F_, device=dev), torch.empty(N, F_, device=dev)
    y = (torch.arange(B) % N).to(dev)
    eta, loss2, gs, gd = torch.empty(B, device=dev), torch.empty(3, device=dev), torch.empty(B, N, device=dev), torch.empty(B, N, device=dev)
    s = _lib.stream()
    return {
        "head_fwd": _time(lambda: L.ign_head_fwd(p(X), p(W), None, p(out), B, F_, N, F_, s), steps),
        "head_bwd_xw": _time(lambda: L.ign_head_bwd(p(g), p(X), p(W), p(gX), p(gW), None, B, F_, N, F_, s), steps),
        "loss": _time(lambda: L.ign_loss_fwd_bwd(p(g), p(out), p(y), p(out), p(eta), p(loss2), p(gs), p(gd), B, N, 1.0, s), steps),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--json", default=None, help="also write the results to this file")
    a = ap.parse_args()
    res = {}
    for N in (3, 39):
        r = {"kernels_ms": kernels_ms(N, 50)}
        if not a.skip_step:
            r["step_ms"] = step_ms(N, a.steps)
        res[f"N={N}"] = r
        print(f"N={N}: {json.dumps(r)}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
