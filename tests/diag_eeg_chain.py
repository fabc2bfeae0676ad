"""Diagnostic: the EEG front end of this tree (data_provider/eeg_chain.py) against a checkout of the parent commit, for all 16 on/off
combinations of --eeg_spatial / --eeg_iir / --eeg_resample / --eeg_preprocess on 6-electrode, 3-subject, T = 400 shards:

  host path      every item of the three splits with --device_standardise off (data_provider -> ds[i]): sha256 of the bytes
  device path    every batch (X, y, mask) of the three prefetched loaders of an Experiment (SBM, batch size 8, seed 0), the training
                 loader under a fixed seed: sha256 of the bytes, and the launches ign_timing counts for the three stage kernels
  records        the files the Experiment wrote beside the checkpoint: eeg_iir.json / eeg_resample.json as bytes, eeg_spatial.npz
                 array by array (a zip member carries its time stamp)
  bench          three interleaved runs of python bench.py --gpus 1 --steps 32 --warmup 8 per tree; the benchmark launches none of
                 this code, so the parent's own range is the margin and nothing is gated

    python tests/diag_eeg_chain.py --parent-tree DIR [--out profiles/eeg_chain_refactor.json] [--no-bench]

One child process per tree and per benchmark run, each under its own time limit; a child uses only what both trees offer (run.get_args,
data_provider, Experiment).  The first child that fails or runs out of time ends the run: nothing more is started on the GPU and no
file is written."""
import argparse
import hashlib
import itertools
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ("spatial", "iir", "resample", "preprocess")
STAGES = ("eeg_spatial", "eeg_iir", "eeg_resample")
LIMIT_S = {"dump": 900, "bench": 600}
BENCH = ["bench.py", "--gpus", "1", "--steps", "32", "--warmup", "8"]


def _flags(on):
    sp, iir, rs, pre = on
    return dict(eeg_spatial="ref=car,align=euclid" if sp else "none", eeg_iir="hp=1,notch=50" if iir else "none",
                eeg_resample="rate=256" if rs else "none",
                eeg_preprocess=("band=8:30,sfreq=256" if rs else "band=8:30") if pre else "none")


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()[:24]


def dump_child(tree, out_path):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import numpy as np
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    import run as driver
    from argparse import Namespace
    from data_provider.data_factory import data_provider
    from eeg_spatial_cases import write_shards
    from exp.experiment_classification import Experiment
    from ign_hip import _lib
    assert os.path.abspath(driver.__file__).startswith(os.path.abspath(tree)), driver.__file__
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        shards = os.path.join(tmp, "shards")
        os.makedirs(shards)
        write_shards(shards, T=400)
        for on in itertools.product((False, True), repeat=4):
            tag = "+".join(n for n, v in zip(ORDER, on) if v) or "none"
            flags = _flags(on)
            for split in ("train", "val", "test"):
                ds, _ = data_provider(Namespace(task_name="classification", data="EEG", root_path=shards, batch_size=8, num_workers=0,
                                                seed=0, device_standardise=False, **flags), split)
                for i in range(len(ds)):
                    x, y = ds[i]
                    out[f"{tag}/host/{split}/{i}"] = _sha(x.numpy(), y.numpy())
            work = os.path.join(tmp, tag)
            os.makedirs(work)
            os.chdir(work)
            argv = ["--model", "SBM", "--data", "EEG", "--data_root", shards, "--dataset", "chisco_npy", "--train_epochs", "1",
                    "--batch_size", "8", "--seed", "0", "--num_workers", "0"]
            for k, v in flags.items():
                argv += ["--" + k, v]
            args = driver.get_args(argv)
            driver.set_seed(0)
            exp = Experiment(args)
            _lib.timing_enable(True)                        # behind the alignment's fit: the prefetcher's launches only
            batches = 0
            for split, loader in (("train", exp.train_loader), ("val", exp.val_loader), ("test", exp.test_loader)):
                torch.manual_seed(7)
                for b, (X, y, mask) in enumerate(loader):
                    out[f"{tag}/device/{split}/{b}"] = _sha(X.cpu().numpy(), y.cpu().numpy(), mask.cpu().numpy())
                    batches += 1
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            out[f"{tag}/launches"] = json.dumps(dict({n: _lib.timing_read(n)[1] for n in STAGES}, batches=batches), sort_keys=True)
            _lib.timing_enable(False)
            names = sorted(f for f in os.listdir(exp.checkpoint_dir) if f.startswith("eeg_"))
            out[f"{tag}/records"] = ",".join(names)
            for f in names:
                path = os.path.join(exp.checkpoint_dir, f)
                if f.endswith(".npz"):
                    z = np.load(path, allow_pickle=False)
                    for k in sorted(z.files):
                        out[f"{tag}/record/{f}/{k}"] = str(z[k].dtype) + str(z[k].shape) + _sha(z[k])
                else:
                    out[f"{tag}/record/{f}"] = hashlib.sha256(open(path, "rb").read()).hexdigest()[:24]
            os.chdir(tmp)
            del exp
    with open(out_path, "w") as f:
        json.dump(out, f)
    print("RESULT " + json.dumps({"entries": len(out)}))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eeg_chain_refactor.json"))
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--child", nargs="+", metavar="KIND")
    a = ap.parse_args()
    if a.child:
        return dump_child(*a.child[1:])
    if not a.parent_tree or not os.path.isdir(a.parent_tree):
        sys.exit("--parent-tree: a checkout of the parent commit with its library built is required")
    trees = {"parent": os.path.abspath(a.parent_tree), "this": ROOT}
    me = [sys.executable, os.path.abspath(__file__), "--child", "dump"]
    res = {"what": "the EEG front end as one chain (data_provider/eeg_chain.py) against a checkout of the parent commit on one MI355X: "
                   "16 on/off combinations of the four --eeg_* flags on 6-electrode, 3-subject, T = 400 shards "
                   "(tests/diag_eeg_chain.py)"}
    with tempfile.TemporaryDirectory() as tmp:
        dumps = {}
        for who, tree in trees.items():
            path = os.path.join(tmp, who + ".json")
            run_child("dump", me + [tree, path], f"dump/{who}")
            dumps[who] = json.load(open(path))
    keys = sorted(set(dumps["parent"]) | set(dumps["this"]))
    different = [k for k in keys if dumps["parent"].get(k) != dumps["this"].get(k)]
    kinds = {kind: sum(1 for k in keys if f"/{kind}" in k) for kind in ("host/", "device/", "launches", "records", "record/")}
    res["bits"] = {"all_equal": not different, "comparisons": len(keys), "different": different,
                   "of_which": {"host_items": kinds["host/"], "device_batches": kinds["device/"], "launch_counts": kinds["launches"],
                                "record_lists": kinds["records"], "record_contents": kinds["record/"]},
                   "launches": {k.split("/")[0]: json.loads(v) for k, v in dumps["this"].items() if k.endswith("/launches")},
                   "what": "sha256 of every host item, of every prefetched batch (X, y, mask) and of every record file, and the launch "
                           "counts of eeg_spatial / eeg_iir / eeg_resample per combination, parent's tree against this tree"}
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
                        "this_ms_per_step_range": rng("this")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    print("bits:", {k: v for k, v in res["bits"].items() if k in ("all_equal", "comparisons", "different")})
    print("bench:", res.get("bench", {}).get("parent_ms_per_step_range"), res.get("bench", {}).get("this_ms_per_step_range"))


if __name__ == "__main__":
    main()
