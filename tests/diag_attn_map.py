"""Diagnostic (not a test): cost of the attention map (ign_attn_probs) and of `output_attention=True` in the Transformer step.
Device events, warm-up, one process.
  (1) ign_attn_probs alone at B 256, H 8, L = S 1000, E 64 (8.19 GB written per call) for every arithmetic, p = 0 and p = 0.1,
      against the write bound 8.19 GB / 6.3 TB/s = 1.3 ms;
  (2) the Transformer baseline's train step (bench.py --config transformer: CHISCO shape, B 256, d_model 512, 8 heads, dropout 0)
      with output_attention False and True, alternated round by round.
For the kernel's own time run it once more under `rocprofv3 --kernel-trace --stats -- python tests/diag_attn_map.py --skip-model`.
Usage: python tests/diag_attn_map.py [--rounds 3] [--out attn_map.json]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import speech_imagery_eeg_amd  # noqa: E402,F401
from ign_hip import _lib, ops  # noqa: E402
from ign_hip.ddp import FlatAdam, FlatParamBucket  # noqa: E402

dev = torch.device("cuda:0")


def timeit(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def map_costs(rounds, n):
    B, L, H, E = 256, 1000, 8, 64
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v = (torch.randn(B, L, H, E, device=dev, generator=g) for _ in range(3))
    lse = torch.empty(B, H, L, device=dev)
    attn = torch.empty(B, H, L, L, device=dev)
    bq, bk = ops.tensor_bound(q), ops.tensor_bound(k)
    # lse of the forward in each arithmetic (the map is then checked for row sums)
    out = torch.empty_like(q)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = (L * H * E, H * E)
    res = {}
    for name, math in (("f16x3", ops.ATTN_MATH_H3), ("bf16x6", ops.ATTN_MATH_X6), ("bf16", ops.ATTN_MATH_BF16), ("f32", ops.ATTN_MATH_F32)):
        if math == ops.ATTN_MATH_H3:
            _lib.check(_lib.lib().ign_attn_fwd_h3(P(q), P(k), P(v), P(out), P(lse), B, L, L, H, E, *st, *st, *st, 0.125, _lib.stream(),
                                                  P(bq), P(bk), P(ops.tensor_bound(v))), "ign_attn_fwd_h3")
        else:
            fwd = {ops.ATTN_MATH_X6: "ign_attn_fwd_x6", ops.ATTN_MATH_BF16: "ign_attn_fwd_bf16", ops.ATTN_MATH_F32: "ign_attn_fwd"}[math]
            _lib.check(getattr(_lib.lib(), fwd)(P(q), P(k), P(v), P(out), P(lse), B, L, L, H, E, *st, *st, *st, 0.125, _lib.stream()), fwd)
        for p in (0.0, 0.1):
            def call(p=p):
                _lib.check(_lib.lib().ign_attn_probs(P(q), P(k), P(lse), P(attn), B, L, L, H, E, *st, *st, 0.125, _lib.stream(), math,
                                                     P(bq), P(bk), p, 0x1234), "ign_attn_probs")
            call()
            torch.cuda.synchronize()
            if p == 0.0:
                rs = attn.view(-1, L)[::977].double().sum(-1)
                print(f"{name}: max |row sum - 1| over a sample of rows {float((rs - 1).abs().max()):.2e}", flush=True)
            for r in range(rounds):
                t = timeit(call, n)
                res.setdefault(f"{name} p={p}", []).append(t)
                print(f"ign_attn_probs {name} p={p} round {r}: {t:.3f} ms = {attn.numel() * 4 / t / 1e9:.2f} TB/s", flush=True)
    return res


def transformer_costs(rounds, n):
    from argparse import Namespace
    from models.Transformer import Model
    cfg = dict(enc_in=122, seq_len=1000, num_class=3, c_out=3, epsilon=1.0, distance_func='euclidean', memory_efficient=False,
               sbm_cls='linear', lambda_reg=0.1, lambda_div=0.1, dnn_type='FCN', model='Transformer', task_name='classification',
               pred_len=0, label_len=0, d_model=512, embed='timeF', freq='h', factor=1, n_heads=8, d_ff=2048, activation='gelu',
               e_layers=2, dropout=0.0)
    B = 256
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, 1000, 122, device=dev, generator=g)
    y = torch.randint(0, 3, (B,), device=dev, generator=g)
    mask = torch.ones(B, 1000, device=dev)
    runs = {}
    for flag in (False, True):
        torch.manual_seed(0)
        m = Model(Namespace(output_attention=flag, **cfg)).to(dev).train()
        bucket = FlatParamBucket(m, 1)
        opt = FlatAdam(bucket, lr=5e-3)

        def step(m=m, bucket=bucket, opt=opt):
            loss = F.cross_entropy(m(x, mask, None, None), y)
            ops.backward(loss)
            opt.step()
            bucket.zero_grad()
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        runs[f"output_attention={flag}"] = step
    res = {}
    for r in range(rounds):
        for name, step in runs.items():
            t = timeit(step, n)
            res.setdefault(name, []).append(t)
            print(f"transformer step, {name}, round {r}: {t:.2f} ms", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"gpu": torch.cuda.get_device_name(0), "ign_attn_probs_ms": map_costs(a.rounds, a.n)}
    if not a.skip_model:
        out["transformer_step_ms"] = transformer_costs(a.rounds, max(4, a.n // 2))
    summary = {f"ign_attn_probs {k} ms (min)": min(v) for k, v in out["ign_attn_probs_ms"].items()}
    for key, ts in out.get("transformer_step_ms", {}).items():
        summary[f"transformer {key} ms (min)"] = min(ts)
    out["summary"] = summary
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
