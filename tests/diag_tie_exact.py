"""Cost of the opt-in exact-tie L1 backward passes (not a test): ign_shapelet_bwd_bank and ign_shapelet_bwd_input_bank with and
without IGN_TIE_EXACT at the benchmark shape (B=256, C=122, T=1000, four groups of K=5 with L = 100 / 200 / 300 / 500), for both
gates.  Warm-up, then the median of repeated event-timed runs; every GPU step is a child process under its own time limit, and
nothing more is started after one fails.  --bench-line records bench.py result lines (parent commit twice, this commit once): the
default path launches the same code as before, so this commit may exceed the parent's slower run by no more than the parent's own
spread.

    python tests/diag_tie_exact.py [--out profiles/tie_exact.json] [--bench-line parent|this FILE ...]
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
SHAPE = dict(B=256, C=122, T=1000, K=5, L=[100, 200, 300, 500])


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


def step_bank(gate):
    """both passes of one bank in the default mode and with the bit, on the same inputs and saved forward"""
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, C, T, K, Ls = SHAPE["B"], SHAPE["C"], SHAPE["T"], SHAPE["K"], SHAPE["L"]
    xn, _ = ops.instance_norm(torch.randn(B, T, C, device=dev))
    ws = [torch.randn(K, C, L, device=dev) for L in Ls]
    thrs = [torch.rand(1, K, C, device=dev) for _ in Ls] if gate & ops.GATE_LTS else [None] * len(Ls)
    res = dict(element_ops=sum(B * C * K * (T - L + 1) * L for L in Ls))
    for label, mode in (("default", ops.DIST_L1 | gate), ("tie_exact", ops.DIST_L1 | gate | ops.TIE_EXACT)):
        bank = ops._Bank(xn, ws, thrs, 1.0, mode, [1] * len(Ls), True)
        P, D = ops._bank_fwd(bank, xn)
        gP = torch.randn(P.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        res[label] = dict(mode=mode, weight_pass=_median_ms(lambda: ops._bank_wgrad(bank, xn, gP, P, D)),
                          input_pass=_median_ms(lambda: ops._bank_xgrad(bank, xn, gP, P, D)))
    for p in ("weight_pass", "input_pass"):
        res[p + "_tie_exact_over_default"] = res["tie_exact"][p]["median_ms"] / res["default"][p]["median_ms"]
    return res


STEPS = {"bank_l1_rbf": lambda: step_bank(0x00), "bank_l1_lts": lambda: step_bank(0x10)}


def _bench_summary(bench):
    """the three ms_per_step values and the rule: this <= slower parent run + (the two parent runs' difference)"""
    par = [b["ms_per_step"] for b in bench.get("parent", []) if b]
    this = [b["ms_per_step"] for b in bench.get("this", []) if b]
    if len(par) < 2 or not this:
        return None
    spread = max(par) - min(par)
    return dict(parent_ms_per_step=par, this_ms_per_step=this, parent_spread_ms=spread, allowed_ms=max(par) + spread,
                within_parent_spread=max(this) <= max(par) + spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tie_exact.json"))
    ap.add_argument("--bench-line", nargs=2, action="append", default=[], metavar=("LABEL", "FILE"),
                    help="record the JSON result line of a bench.py run (its last line starting with '{') under LABEL")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(STEPS[a.step]()))
        return
    res = dict(shape=SHAPE)
    for name in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=300)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            res[name] = dict(failed=r.returncode, stderr=r.stderr[-2000:])
            break                                   # nothing more is started on the GPU after a failed step
        res[name] = json.loads(line[-1][7:])
        print(name, json.dumps(res[name]), flush=True)
    for label, path in a.bench_line:
        lines = [l for l in open(path).read().splitlines() if l.startswith("{")]
        res.setdefault("bench", {}).setdefault(label, []).append(json.loads(lines[-1]) if lines else None)
    if "bench" in res:
        res["bench_summary"] = _bench_summary(res["bench"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    if any("failed" in v for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
