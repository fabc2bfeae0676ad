"""Diagnostic: csrc/ign_optim.hip (one Adam kernel, one launcher) against a libign_hip.so built from the parent commit -- the eight
entry points that work on the flat buffers (four ign_adam_step*, two ign_gather_flat*, ign_grad_norm_clip, ign_scale_flat):

  bit identity   seeded inputs, three calls, at two flat lengths (4416 and the IGN-default bucket's own at the benchmark shape):
                 the outputs of a parent-library process and of a new-library process, compared byte for byte
  kernel time    the same calls at the IGN-default length: device events around 200 back-to-back calls, median of 7 windows, in
                 processes that alternate parent, new, parent, new; the margin of an entry is the parent's own spread in this run
  whole step     tests/diag_clip_step.py on this tree and on a checkout of the parent (--parent-tree), side by side

    python tests/diag_optim_refactor.py --parent-lib PATH [--parent-tree DIR] [--out profiles/optim_refactor.json]

Every measurement runs in a child process of its own under its own time limit, and each child loads exactly one library; the first
child that fails or runs out of time ends the run (nothing more is started on the GPU) and no file is written.  The "what" /
"static" / "static_notes" entries of an existing --out file are kept."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_LIB = os.path.join(ROOT, "speech-imagery-eeg_amd", "csrc", "libign_hip.so")
ENTRIES = ("ign_adam_step", "ign_adam_step_clip", "ign_adam_step_dev", "ign_adam_step_clip_dev", "ign_gather_flat",
           "ign_gather_flat_acc", "ign_grad_norm_clip", "ign_scale_flat")
BENCH = dict(enc_in=122, seq_len=1000, num_class=3)
CALLS, WARMUP, WINDOW, WINDOWS = 3, 20, 200, 7
LIMIT_S = {"layout": 180, "bits": 300, "time": 300, "step": 1500}


def layout_child():
    """the two flat layouts (CPU only, no library): the three-parameter bucket of tests/test_gpu_clip.py and IGN-default's"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from conftest import make_cfg
    from ign_hip.ddp import FlatParamBucket
    from models.InterpGN import InterpGN
    torch.manual_seed(0)
    b = FlatParamBucket(InterpGN(make_cfg(**BENCH)), 1)
    out = {"n4416": {"n": 4416, "sizes": [1, 130, 4099], "offsets": [0, 64, 256]},
           "ign_default": {"n": b.flat_grad.numel(), "sizes": [p.numel() for p in b.params], "offsets": list(b.offsets)}}
    print("RESULT " + json.dumps(out))


def make_calls(lib_path, lay):
    """entry -> (one call of it, the tensors it writes); the inputs depend only on the layout"""
    sys.path.insert(0, ROOT)
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip._lib import SIGNATURES
    L = ctypes.CDLL(lib_path)
    for name in ENTRIES + ("ign_grad_norm_workspace_bytes", "ign_last_error"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = SIGNATURES[name]
    dev = torch.device("cuda:0")
    n, sizes = lay["n"], lay["sizes"]
    gen = torch.Generator().manual_seed(n)
    randn = lambda k=n: torch.randn(k, generator=gen).to(dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    grad, coef = randn(), torch.tensor([0.37], device=dev)

    def checked(name, *args):
        rc = getattr(L, name)(*args, stream)
        if rc != 0:
            raise RuntimeError(f"{name}: rc {rc}: {L.ign_last_error()}")

    def adam(name):
        p, m, v = randn(), randn(), torch.rand(n, generator=gen).to(dev)
        step_dev, bc_dev = torch.zeros(1, device=dev, dtype=torch.int32), torch.zeros(2, device=dev)
        count = [0]

        def call():
            count[0] += 1
            args = [ptr(p), ptr(grad), ptr(m), ptr(v), n, 5e-3, 0.9, 0.999, 1e-8]
            args += [ptr(step_dev), ptr(bc_dev)] if name.endswith("_dev") else [count[0]]
            checked(name, *(args + ([ptr(coef)] if "_clip" in name else [])))
        return call, [p, m, v, step_dev, bc_dev]

    def gather(name):
        flat, srcs = randn(), [randn(s) for s in sizes]
        k = len(srcs)
        src = (ctypes.c_void_p * k)(*[s.data_ptr() for s in srcs])
        off = (ctypes.c_longlong * k)(*lay["offsets"])
        cnt = (ctypes.c_longlong * k)(*sizes)
        return (lambda keep=srcs: checked(name, src, off, cnt, k, ptr(flat))), [flat]      # `keep`: the table holds raw addresses

    def norm(name):
        out2 = torch.full((2,), -1.0, device=dev)
        ws = torch.zeros(L.ign_grad_norm_workspace_bytes(n) // 4, device=dev)
        return (lambda: checked(name, ptr(grad), n, 0.5, ptr(out2), ptr(ws))), [out2, ws]

    def scale(name):
        buf = randn()
        return (lambda: checked(name, ptr(buf), n, ptr(coef))), [buf]

    makers = {"ign_gather_flat": gather, "ign_gather_flat_acc": gather, "ign_grad_norm_clip": norm, "ign_scale_flat": scale}
    return torch, {name: makers.get(name, adam)(name) for name in ENTRIES}


def bits_child(lib_path, layouts, outdir):
    for tag, lay in json.load(open(layouts)).items():
        torch, calls = make_calls(lib_path, lay)
        for name, (call, outs) in calls.items():
            for _ in range(CALLS):
                call()
            torch.cuda.synchronize()
            with open(os.path.join(outdir, f"{tag}.{name}.bin"), "wb") as f:
                for t in outs:
                    f.write(t.cpu().numpy().tobytes())
    print("RESULT {}")


def time_child(lib_path, layouts):
    torch, calls = make_calls(lib_path, json.load(open(layouts))["ign_default"])
    out = {}
    for name, (call, _) in calls.items():
        for _ in range(WARMUP):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(WINDOWS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(WINDOW):
                call()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / WINDOW)
        out[name] = round(statistics.median(us), 3)
    print("RESULT " + json.dumps(out))


def run_child(kind, cmd, what):
    """-> the child's RESULT; ends the whole run at the first child that fails or runs out of time"""
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[kind])
    except subprocess.TimeoutExpired:
        sys.exit(f"{what}: no result within {LIMIT_S[kind]} s; stopping")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.exit(f"{what}: exit status {r.returncode}; stopping\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
    print(what, "ok", flush=True)
    return json.loads(line[-1][len("RESULT "):])


def whole_step(tree, tmp, tag):
    """tests/diag_clip_step.py of `tree` (it starts one child per row itself) -> its rows"""
    out = os.path.join(tmp, f"clip_step_{tag}.json")
    cmd = [sys.executable, os.path.join(tree, "tests", "diag_clip_step.py"), "--out", out]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S["step"], cwd=tree)
    except subprocess.TimeoutExpired:
        sys.exit(f"diag_clip_step ({tag}): not done within {LIMIT_S['step']} s; stopping")
    if r.returncode != 0 or not os.path.exists(out):
        sys.exit(f"diag_clip_step ({tag}): exit status {r.returncode}; stopping\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
    print(f"diag_clip_step ({tag}) ok", flush=True)
    return json.load(open(out))["rows"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libign_hip.so built from the parent commit's csrc")
    ap.add_argument("--parent-tree", help="checkout of the parent commit with its library built: adds the whole-step comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_refactor.json"))
    ap.add_argument("--child", nargs="+", metavar="KIND")
    a = ap.parse_args()
    if a.child:
        return {"layout": layout_child, "bits": bits_child, "time": time_child}[a.child[0]](*a.child[1:])
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: a libign_hip.so built from the parent commit is required")
    libs = {"parent": os.path.abspath(a.parent_lib), "new": NEW_LIB}
    me = [sys.executable, os.path.abspath(__file__), "--child"]
    out = {}
    if os.path.exists(a.out):
        out = {k: v for k, v in json.load(open(a.out)).items() if k in ("what", "static", "static_notes")}
    with tempfile.TemporaryDirectory() as tmp:
        layouts = os.path.join(tmp, "layouts.json")
        lay = run_child("layout", me + ["layout"], "layout")
        json.dump(lay, open(layouts, "w"))
        for tag, path in libs.items():
            os.makedirs(os.path.join(tmp, tag))
            run_child("bits", me + ["bits", path, layouts, os.path.join(tmp, tag)], f"bits/{tag}")
        out["bit_identity"] = {"calls": CALLS, "flat_floats": {k: v["n"] for k, v in lay.items()}, "comparisons": []}
        for name in sorted(os.listdir(os.path.join(tmp, "parent"))):
            old, new = (open(os.path.join(tmp, tag, name), "rb").read() for tag in libs)
            out["bit_identity"]["comparisons"].append({"output": name[:-len(".bin")], "bytes": len(old), "equal": old == new,
                                                       "sha256_16": hashlib.sha256(new).hexdigest()[:16]})
        out["bit_identity"]["all_equal"] = all(c["equal"] for c in out["bit_identity"]["comparisons"])
        runs = {"parent": [], "new": []}
        for i in range(2):
            for tag, path in libs.items():                     # parent, new, parent, new
                runs[tag].append(run_child("time", me + ["time", path, layouts], f"time/{tag}/{i}"))
        rows = {}
        for name in ENTRIES:
            old, new = [r[name] for r in runs["parent"]], [r[name] for r in runs["new"]]
            spread = max(old) / min(old) - 1.0
            rows[name] = {"parent_median_us": old, "new_median_us": new, "parent_spread": round(spread, 4),
                          "passes": max(new) <= max(old) * (1.0 + spread)}
        out["kernel_time"] = {"what": f"us per call at {lay['ign_default']['n']} floats: device events around {WINDOW} back-to-back "
                                      f"calls, median of {WINDOWS} windows per process; new passes if its worse median <= the "
                                      "parent's worse median * (1 + parent_spread)", "entries": rows}
        if a.parent_tree:
            step = {tag: whole_step(tree, tmp, tag) for tag, tree in (("new", ROOT), ("parent", os.path.abspath(a.parent_tree)))}
            out["whole_step"] = {"what": "tests/diag_clip_step.py on both trees in one run; ms_per_step is reported, not gated", "rows": [
                {"shape": n["shape"], "config": n["config"], "parent_ms_per_step": p["ms_per_step"], "new_ms_per_step": n["ms_per_step"],
                 "parent_launches_per_step": p["launches_per_step"], "new_launches_per_step": n["launches_per_step"]}
                for p, n in zip(step["parent"], step["new"])]}
            out["whole_step"]["launches_equal"] = all(r["parent_launches_per_step"] == r["new_launches_per_step"]
                                                      for r in out["whole_step"]["rows"])
    out["gpu"] = "measured on one MI355X (tests/diag_optim_refactor.py)"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)
    for name, r in out["kernel_time"]["entries"].items():
        print(name, r)
    print("bit identity:", out["bit_identity"]["all_equal"], "| whole-step launches equal:",
          out.get("whole_step", {}).get("launches_equal"))


if __name__ == "__main__":
    main()
