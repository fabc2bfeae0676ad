"""Diagnostic: the explanation host path of this tree (utils/explain.py) against a checkout of the parent commit on one MI355X.  The
kernels are the same in both trees, so every difference is a host-path bug.

  bits     seeded SBM, LTS, InterpGN(FCN) and FCN at (4, 100, 6), N = 4 -- and SBM / InterpGN with mask_padding on under a padding mask
           of lengths [100, 37, 0, 64]: input_saliency and evidence_map for every accepted explain; faithfulness_curves under
           explain=sbm with attr=evidence+saliency+random+occlusion, steps=4, both modes, both units, both fills, and under
           explain=model with attr=occlusion+random; occlusion_map under model / sbm / gated / dnn with window=20, stride=10,
           groups each and all, both scores, rows=7; run.py --test_only on SYNTH data with --evidence, --faithfulness and --occlusion
           on.  Per call: the sha256 of every returned tensor (a refusal: its type and text) and of every written file's arrays, and
           how often each ops.* function involved was called
  time     one call of each of the four explainers on the InterpGN: the median of 20 calls after 3 warm-up calls, a device synchronise
           around each; the parent is timed twice, and the distance between its two medians is the margin
  bench    three interleaved runs of python bench.py --gpus 1 --steps 32 --warmup 8 per tree; the benchmark launches none of this code

    python tests/diag_explain.py --parent-tree DIR [--out profiles/explain_refactor.json] [--no-bench]

One child process per tree and per run, each under its own time limit; a child uses only what both trees offer.  The first child that
fails or runs out of time ends the run: nothing more is started on the GPU and no file is written."""
import argparse
import hashlib
import itertools
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = {"dump": 420, "time": 240, "bench": 300}
BENCH = ["bench.py", "--gpus", "1", "--steps", "32", "--warmup", "8"]
OPS = ("shapelet_evidence", "fcn_cam", "cam_spread", "rank_threshold", "perturb", "occlude", "occlusion_spread")
ACCEPTED = {"SBM": ("sbm",), "LTS": ("sbm",), "InterpGN": ("sbm", "gated", "dnn"), "FCN": ("dnn",)}
B, T, C, N = 4, 100, 6, 4
LENGTHS = [100, 37, 0, 64]


def _setup(tree):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    import run as driver
    assert os.path.abspath(driver.__file__).startswith(os.path.abspath(tree)), driver.__file__
    return torch, driver


def _model(kind, torch, **kw):
    from conftest import make_cfg
    from models.FullyConvNet import FullyConvNetwork
    from models.InterpGN import InterpGN
    from models.Shapelet import DistThresholdSBM, ShapeBottleneckModel
    torch.manual_seed(0)
    cls = dict(SBM=ShapeBottleneckModel, LTS=DistThresholdSBM, InterpGN=InterpGN, FCN=FullyConvNetwork)[kind]
    return cls(make_cfg(**kw)).to("cuda:0").train()


def _digest(torch, value):
    """a tensor -> dtype, shape and the sha256 of its bytes; a result record -> that of every field"""
    import dataclasses
    if value is None or isinstance(value, (str, int, float)):
        return repr(value)
    if torch.is_tensor(value):
        a = value.detach().cpu().contiguous().numpy()
        return f"{a.dtype}{a.shape}" + hashlib.sha256(a.tobytes()).hexdigest()[:24]
    if dataclasses.is_dataclass(value):
        value = {f.name: getattr(value, f.name) for f in dataclasses.fields(value)}
    elif hasattr(value, "_asdict"):
        value = value._asdict()
    if isinstance(value, dict):
        return {str(k): _digest(torch, v) for k, v in value.items()}
    raise TypeError(type(value))


def dump_child(tree, out_path):
    torch, driver = _setup(tree)
    import numpy as np
    from ign_hip import ops
    from utils.evidence import evidence_map
    from utils.faithfulness import faithfulness_curves
    from utils.occlusion import occlusion_map
    from utils.saliency import input_saliency
    counts = dict.fromkeys(OPS, 0)

    def counted(name, fn):
        def wrapper(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return wrapper

    for name in OPS:
        setattr(ops, name, counted(name, getattr(ops, name)))
    out = {}

    def record(key, fn):
        before = dict(counts)
        try:
            got = _digest(torch, fn())
        except (TypeError, ValueError, RuntimeError) as err:                  # a refusal is a result too: both trees word it alike
            got = f"{type(err).__name__}: {err}"
        out[key] = json.dumps(got, sort_keys=True)
        out[key + "/calls"] = json.dumps({n: counts[n] - before[n] for n in OPS if counts[n] != before[n]}, sort_keys=True)

    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(1)).to("cuda:0")
    ragged = (torch.arange(T)[None, :] < torch.tensor(LENGTHS)[:, None]).float().to("cuda:0")
    for kind, padded in (("SBM", False), ("LTS", False), ("InterpGN", False), ("FCN", False), ("SBM", True), ("InterpGN", True)):
        model = _model(kind, torch, mask_padding=True) if padded else _model(kind, torch)
        mask = ragged if padded else None
        xm = x * ragged[:, :, None] if padded else x
        tag = kind + ("+mask" if padded else "")
        for explain in ACCEPTED[kind]:
            record(f"{tag}/saliency/{explain}", lambda: input_saliency(model, xm, explain=explain))
            record(f"{tag}/evidence/{explain}", lambda: evidence_map(model, xm, explain=explain, mask=mask))
        if "sbm" in ACCEPTED[kind]:
            for mode, unit, fill in itertools.product(("deletion", "insertion"), ("cell", "time"), ("mean", "zero")):
                record(f"{tag}/faithfulness/sbm/{mode}/{unit}/{fill}", lambda: faithfulness_curves(
                    model, xm, mask=mask, explain="sbm", attributions=("evidence", "saliency", "random", "occlusion"), steps=4, mode=mode,
                    unit=unit, fill=fill, seed=5, window=20, stride=10))
        record(f"{tag}/faithfulness/model", lambda: faithfulness_curves(model, xm, mask=mask, explain="model",
                                                                        attributions=("occlusion", "random"), steps=4, window=20, stride=10))
        for explain, groups, score in itertools.product(("model",) + ACCEPTED[kind], ("each", "all"), ("logit", "prob")):
            record(f"{tag}/occlusion/{explain}/{groups}/{score}", lambda: occlusion_map(
                model, xm, mask=mask, explain=explain, window=20, stride=10, groups=groups, score=score, rows=7))
        assert model.training and not any(p.grad is not None for p in model.parameters())
    # the driver: a seeded, untrained InterpGN as the checkpoint, then run.py --test_only with the three flags on
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        argv = ["--data", "SYNTH", "--synthetic", "24,6,100,4", "--model", "InterpGN", "--dnn_type", "FCN", "--batch_size", "8", "--seed", "0",
                "--gating_value", "0.5", "--dataset", "diag"]
        driver.set_seed(0)
        exp = driver.exp_dict["classification"](args=driver.get_args(argv))
        os.makedirs(exp.checkpoint_dir, exist_ok=True)
        torch.save(exp.model.state_dict(), os.path.join(exp.checkpoint_dir, "checkpoint.pth"))
        folder = os.path.abspath(exp.checkpoint_dir)
        del exp
        before = dict(counts)
        driver.main(argv + ["--test_only", "--evidence", "gated", "--faithfulness", "explain=gated,steps=3,seed=2",
                            "--occlusion", "explain=model,window=50,stride=25,groups=each"])
        out["driver/calls"] = json.dumps({n: counts[n] - before[n] for n in OPS}, sort_keys=True)
        names = sorted(f for f in os.listdir(folder) if f.split(".")[0] in ("evidence", "faithfulness", "occlusion"))
        out["driver/files"] = ",".join(names)
        for f in names:
            path = os.path.join(folder, f)
            if f.endswith(".npz"):
                z = np.load(path, allow_pickle=False)
                for k in sorted(z.files):
                    out[f"driver/{f}/{k}"] = _digest(torch, torch.from_numpy(np.ascontiguousarray(z[k])))
            else:
                out[f"driver/{f}"] = hashlib.sha256(open(path, "rb").read()).hexdigest()[:24]
        os.chdir(ROOT)
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump(out, f)
    print("RESULT " + json.dumps({"entries": len(out)}))


def time_child(tree, out_path):
    torch, _ = _setup(tree)
    import statistics
    import time
    from utils.evidence import evidence_map
    from utils.faithfulness import faithfulness_curves
    from utils.occlusion import occlusion_map
    from utils.saliency import input_saliency
    model = _model("InterpGN", torch)
    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(1)).to("cuda:0")
    calls = {"input_saliency": lambda: input_saliency(model, x, explain="gated"),
             "evidence_map": lambda: evidence_map(model, x, explain="gated"),
             "faithfulness_curves": lambda: faithfulness_curves(model, x, explain="sbm", steps=4),
             "occlusion_map": lambda: occlusion_map(model, x, explain="model", window=20, stride=10, groups="each", rows=64)}
    out = {}
    for name, fn in calls.items():
        ms = []
        for i in range(23):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}
    with open(out_path, "w") as f:
        json.dump(out, f)
    print("RESULT " + json.dumps(out))


def run_child(kind, cmd, what, cwd=None):
    """-> the child's stdout; ends the whole run at the first child that fails or runs out of time"""
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[kind], cwd=cwd)
    except subprocess.TimeoutExpired:
        sys.exit(f"{what}: no result within {LIMIT_S[kind]} s; stopping")
    if r.returncode != 0:
        sys.exit(f"{what}: exit status {r.returncode}; stopping\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    print(what, "ok", flush=True)
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_refactor.json"))
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--child", nargs="+", metavar="KIND")
    a = ap.parse_args()
    if a.child:
        return {"dump": dump_child, "time": time_child}[a.child[0]](*a.child[1:])
    if not a.parent_tree or not os.path.isdir(a.parent_tree):
        sys.exit("--parent-tree: a checkout of the parent commit with its library built is required")
    trees = {"parent": os.path.abspath(a.parent_tree), "this": ROOT}
    me = [sys.executable, os.path.abspath(__file__), "--child"]
    res = {"what": "the explanation host path (utils/explain.py) against a checkout of the parent commit on one MI355X: SBM, LTS, "
                   "InterpGN(FCN) and FCN at (4, 100, 6), N = 4, without and with a padding mask (tests/diag_explain.py)"}
    with tempfile.TemporaryDirectory() as tmp:
        dumps = {}
        for who, tree in trees.items():
            path = os.path.join(tmp, who + ".json")
            run_child("dump", me + ["dump", tree, path], f"dump/{who}")
            dumps[who] = json.load(open(path))
        times = []
        for who in ("parent", "this", "parent"):                             # the parent twice: its own spread is the margin
            path = os.path.join(tmp, "time.json")
            run_child("time", me + ["time", trees[who], path], f"time/{who}")
            times.append({"who": who, "calls": json.load(open(path))})
    keys = sorted(set(dumps["parent"]) | set(dumps["this"]))
    different = [k for k in keys if dumps["parent"].get(k) != dumps["this"].get(k)]
    refusals = sorted(k for k in keys if dumps["this"].get(k, "").startswith('"') and "Error: " in dumps["this"][k])
    res["bits"] = {"all_equal": not different, "comparisons": len(keys), "different": different,
                   "of_which": {"call_counts": sum(1 for k in keys if k.endswith("/calls")),
                                "driver": sum(1 for k in keys if k.startswith("driver/")), "refusals": len(refusals)},
                   "refused_alike": refusals, "driver_calls": json.loads(dumps["this"]["driver/calls"]),
                   "what": "sha256 of every tensor the four explainers return and of every array run.py writes, and the calls of "
                           + ", ".join("ops." + n for n in OPS) + " per explainer call, parent's tree against this tree"}
    med = lambda i, name: times[i]["calls"][name]["median_ms"]
    res["time"] = {"what": "median ms of 20 calls after 3 warm-up calls, a device synchronise around each call, InterpGN(FCN) at (4, 100, 6); "
                           "the parent is timed twice and the distance between its two medians is the margin", "runs": times,
                   "summary": {name: {"parent_ms": [med(0, name), med(2, name)], "this_ms": med(1, name),
                                      "margin_ms": abs(med(0, name) - med(2, name)),
                                      "this_above_slower_parent_ms": med(1, name) - max(med(0, name), med(2, name))}
                               for name in times[0]["calls"]}}
    if not a.no_bench:
        runs = []
        for i in (1, 2, 3):
            for who, tree in trees.items():                 # parent, this, parent, this, ...
                line = [l for l in run_child("bench", [sys.executable] + BENCH, f"bench/{who}/{i}", cwd=tree).splitlines()
                        if l.startswith("{") and '"metric"' in l]
                if not line:
                    sys.exit(f"bench/{who}/{i}: no result line; stopping")
                r = json.loads(line[-1])
                runs.append({"who": who, "run": i, "value": r.get("value"), "ms_per_step": r.get("ms_per_step")})
        rng = lambda who: [f([r["ms_per_step"] for r in runs if r["who"] == who]) for f in (min, max)]
        res["bench"] = {"what": "python " + " ".join(BENCH) + ", interleaved with the parent's tree, three runs each; the benchmark "
                                "launches none of this code", "runs": runs, "parent_ms_per_step_range": rng("parent"),
                        "this_ms_per_step_range": rng("this"),
                        "ranges_overlap": rng("this")[0] <= rng("parent")[1] and rng("parent")[0] <= rng("this")[1]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    print("bits:", {k: v for k, v in res["bits"].items() if k in ("all_equal", "comparisons", "different", "of_which")})
    print("time:", json.dumps(res["time"]["summary"]))
    print("bench:", res.get("bench", {}).get("parent_ms_per_step_range"), res.get("bench", {}).get("this_ms_per_step_range"))


if __name__ == "__main__":
    main()
