"""Diagnostic (not a test): cost of attention dropout inside the fused kernels.  Device events, warm-up, p = 0 and p = 0.1
alternated round by round in one process.
  (1) attention forward + backward at B 256, L = S 1000, H 8, E 64 for the f16x3 (default) and f32 arithmetics;
  (2) the Transformer baseline's train step (bench.py --config transformer: CHISCO shape, B 256, d_model 512, 8 heads) at
      dropout 0, at attention dropout 0.1 alone (the other dropouts 0) and at --dropout 0.1 (every dropout of the model).
Usage: python tests/diag_attn_dropout.py [--rounds 3] [--out attn_dropout.json]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import speech_imagery_eeg_amd  # noqa: E402,F401
from ign_hip import ops  # noqa: E402
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


def attention_costs(rounds, n):
    B, L, H, E = 256, 1000, 8, 64
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v = (torch.randn(B, L, H, E, device=dev, generator=g).requires_grad_(True) for _ in range(3))
    go = torch.randn(B, L, H, E, device=dev, generator=g)
    res = {}
    for amath in ("f16x3", "f32"):
        ops.ATTN_MATH, ops.GEMM_MATH = ("bf16x6", "f16x3") if amath == "f16x3" else ("f32", "bf16x6")
        for p in (0.0, 0.1):
            def fwd_bwd(p=p):
                o = ops.attention(q, k, v, 0.125, dropout_p=p)
                torch.autograd.grad(o, (q, k, v), go)
            for _ in range(2):
                fwd_bwd()
            torch.cuda.synchronize()
        for r in range(rounds):
            for p in (0.0, 0.1):
                def fwd(p=p):
                    with torch.no_grad():
                        ops.attention(q, k, v, 0.125, dropout_p=p)

                def fwd_bwd(p=p):
                    o = ops.attention(q, k, v, 0.125, dropout_p=p)
                    torch.autograd.grad(o, (q, k, v), go)
                tf, tfb = timeit(fwd, n), timeit(fwd_bwd, n)
                res.setdefault(f"{amath} p={p}", []).append({"fwd_ms": tf, "fwd_bwd_ms": tfb})
                print(f"attention {amath} p={p} round {r}: fwd {tf:.3f} ms, fwd+bwd {tfb:.3f} ms", flush=True)
    ops.ATTN_MATH, ops.GEMM_MATH = "bf16x6", "f16x3"
    return res


def transformer_costs(rounds, n):
    from argparse import Namespace
    from models.Transformer import Model
    from layers.SelfAttention_Family import FullAttention
    cfg = dict(enc_in=122, seq_len=1000, num_class=3, c_out=3, epsilon=1.0, distance_func='euclidean', memory_efficient=False,
               sbm_cls='linear', lambda_reg=0.1, lambda_div=0.1, dnn_type='FCN', model='Transformer', task_name='classification',
               pred_len=0, label_len=0, output_attention=False, d_model=512, embed='timeF', freq='h', factor=1, n_heads=8,
               d_ff=2048, activation='gelu', e_layers=2)
    B = 256
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, 1000, 122, device=dev, generator=g)
    y = torch.randint(0, 3, (B,), device=dev, generator=g)
    mask = torch.ones(B, 1000, device=dev)
    runs = {}
    for name, p in (("dropout 0", 0.0), ("attention dropout 0.1", 0.1), ("dropout 0.1", 0.1)):
        torch.manual_seed(0)
        m = Model(Namespace(dropout=p, **cfg))
        if name.startswith("attention"):
            for mod in m.modules():
                if isinstance(mod, torch.nn.Dropout):
                    mod.p = 0.0
            for mod in m.modules():
                if isinstance(mod, FullAttention):
                    mod.dropout.p = p
        m = m.to(dev).train()
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
        runs[name] = step
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
    out = {"gpu": torch.cuda.get_device_name(0), "attention": attention_costs(a.rounds, a.n)}
    if not a.skip_model:
        out["transformer_step_ms"] = transformer_costs(a.rounds, max(4, a.n // 2))
    summary = {}
    for key, rows in out["attention"].items():
        summary[f"attention {key} fwd+bwd ms (min)"] = min(r["fwd_bwd_ms"] for r in rows)
        summary[f"attention {key} fwd ms (min)"] = min(r["fwd_ms"] for r in rows)
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
