"""Bits of the loss tail: every output of ops.ign_loss, ops.ign_crps_loss, ops.crps_loss and ops.gini_gate (forward and backward,
gating_value None and 0.3) for fixed seeds at N in {2, 5, 16, 17, 65, 256} x B in {1, 257, 1025}, and of ops.ign_loss under each of
its label rules (ce_cases below), written to one .npz.  Run it on two builds on the same machine and compare the files: a change that
only moves or restates the kernels leaves every array bitwise equal.  Uses the public ops functions only.  A measuring script, not a
test; tests/test_gpu_loss_tail_bits.py takes its cases from here.

    python tests/diag_loss_tail.py --out tail.npz
    python tests/diag_loss_tail.py --compare a.npz b.npz        (no device needed; exit status 1 when an array differs)
    python tests/diag_loss_tail.py --digest bits.json           (sha256 of every input and output of ce_cases: tests/golden/loss_tail_bits.json)
    python tests/diag_loss_tail.py --time times.json [--runs 3] (the three CE entry points, thread-per-row and wave-per-row, ms per launch)"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

NS, BS = (2, 5, 16, 17, 65, 256), (1, 257, 1025)      # B = 1025 crosses the 1024-row tiles of the wide CE tail and the CRPS tails

# ---------------------------------------------------------------- the CE tail under its three label rules
# N: 2 smallest, 16 | 17 the last thread-per-row and the first wave-per-row width, 65 one lane in a second chunk, 256 every chunk full
# B: 257 gives thread 0 a second row and wraps the 16 waves; 1025 crosses the 1024-row LDS tile of the wave-per-row layout and gives
#    the pre-pass of the weighted rules a second row per thread
CE_NS, CE_BS = (2, 3, 16, 17, 65, 256), (1, 5, 257, 1025)
CE_BETA, CE_REG = 0.7, 0.125
# name -> (class weights, label smoothing, soft labels); "plain" is the call without options
CE_OPTIONS = {"plain": (False, 0.0, False), "w": (True, 0.0, False), "w_eps": (True, 0.1, False), "eps": (False, 0.1, False),
              "mix_w_eps": (True, 0.1, True), "mix": (False, 0.0, True)}
CE_OUTPUTS = ("loss", "out", "eta", "gsbm", "gdnn")
CE_CLAMP = "clamp_n3_b5"                              # labels and lam out of range, for the two rules that clamp them


def ce_inputs(B, N):
    """-> host tensors by name, the conventions of tests/test_gpu_mix_loss.py::_case: logits randn * 3, class 0 heavy (and never absent
    from the first labels), lam uniform with an exact 0 and an exact 1 when B > 2."""
    g = torch.Generator().manual_seed(1000 * N + B)
    s, d = torch.randn(B, N, generator=g) * 3, torch.randn(B, N, generator=g) * 3
    ya = torch.randint(0, N - 1, (B,), generator=g)
    ya[0] = 0
    yb = torch.randint(0, N, (B,), generator=g)
    lam = torch.rand(B, generator=g)
    if B > 2:
        lam[1], lam[2] = 0.0, 1.0
    w = 0.2 + 4.8 * torch.rand(N, generator=g)
    w[0] = 50.0 * w[1:].max()
    return dict(s=s, d=d, ya=ya, yb=yb, lam=lam, w=w)


def ce_cases():
    """-> [(shape tag, inputs, option names)]: the grid, then the clamp case (never under "plain": that rule does not clamp, the read
    would be out of bounds)."""
    cases = [(f"n{N}_b{B}", ce_inputs(B, N), tuple(CE_OPTIONS)) for N in CE_NS for B in CE_BS]
    x = ce_inputs(5, 3)
    x["ya"][3], x["ya"][4], x["yb"][4], x["yb"][1], x["lam"][0], x["lam"][3] = 7, -2, -2, 3, 1.5, -0.25
    return cases + [(CE_CLAMP, x, ("w_eps", "mix_w_eps"))]


def ce_run(ops, dev, x, option):
    """-> the CE_OUTPUTS of ops.ign_loss + ops.backward on the inputs `x` under CE_OPTIONS[option], as device tensors"""
    weights, eps, soft = CE_OPTIONS[option]
    s, d = x["s"].to(dev).requires_grad_(True), x["d"].to(dev).requires_grad_(True)
    kw = {}
    if option != "plain":
        kw.update(class_weight=x["w"].to(dev) if weights else None, label_smoothing=eps)
    if soft:
        kw.update(y_b=x["yb"].to(dev), lam=x["lam"].to(dev))
    loss, out, eta = ops.ign_loss(s, d, x["ya"].to(dev), CE_BETA, reg=torch.tensor([CE_REG], device=dev), **kw)
    ops.backward(loss)
    return loss.detach(), out, eta, s.grad, d.grad


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def ce_digests(ops, dev, x, options):
    """-> {"inputs": {name: sha256}, "outputs": {option: {name: sha256}}} of one entry of ce_cases()"""
    return dict(inputs={k: sha(v) for k, v in x.items()},
                outputs={o: dict(zip(CE_OUTPUTS, map(sha, ce_run(ops, dev, x, o)))) for o in options})


def digest(path):
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    dev = torch.device("cuda:0")
    src = open(os.path.join(ROOT, "speech-imagery-eeg_amd", "csrc", "ign_loss.hip"), "rb").read()
    doc = dict(ign_loss_hip_blob=hashlib.sha1(b"blob %d\0" % len(src) + src).hexdigest(), hip=torch.version.hip, torch=torch.__version__,
               beta=CE_BETA, reg=CE_REG,
               cases={tag: ce_digests(ops, dev, x, options) for tag, x, options in ce_cases()})
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(doc['cases'])} cases -> {path}")


def dump(path):
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    dev = torch.device("cuda:0")
    arrays = {}

    def keep(tag, names, tensors):
        for n, t in zip(names, tensors):
            arrays[f"{tag}.{n}"] = t.detach().cpu().numpy()

    for N in NS:
        e = torch.linspace(-2, 2, N + 1, dtype=torch.float64)
        e[-1] = float("inf")
        edges = e[1:].to(dev)
        for B in BS:
            g = torch.Generator().manual_seed(1000 * N + B)
            s0, d0 = (torch.randn(B, N, generator=g) * 2).to(dev), (torch.randn(B, N, generator=g) * 2).to(dev)
            y = torch.randint(0, N, (B,), generator=g).to(dev)
            t = (torch.randn(B, generator=g) * 1.5).to(dev)
            gout, geta = torch.randn(B, N, generator=g).to(dev), torch.randn(B, 1, generator=g).to(dev)
            reg = torch.tensor([0.125], device=dev)
            tag = f"n{N}_b{B}"
            for name, call in (("ign_loss", lambda s, d: ops.ign_loss(s, d, y, 0.7, reg=reg)),
                               ("ign_crps_loss", lambda s, d: ops.ign_crps_loss(s, d, t, edges, 0.7, reg=reg))):
                s, d = s0.clone().requires_grad_(True), d0.clone().requires_grad_(True)
                loss, out, eta = call(s, d)
                ops.backward(loss)
                keep(f"{name}.{tag}", ("loss", "out", "eta", "gsbm", "gdnn"), (loss, out, eta, s.grad, d.grad))
            s = s0.clone().requires_grad_(True)
            loss = ops.crps_loss(s, t, edges)
            ops.backward(loss)
            keep(f"crps_loss.{tag}", ("loss", "grad"), (loss, s.grad))
            for gv in (None, 0.3):
                s, d = s0.clone().requires_grad_(True), d0.clone().requires_grad_(True)
                out, eta = ops.gini_gate(s, d, gv)
                torch.autograd.backward([out, eta], [gout, geta])
                keep(f"gini_gate_{gv}.{tag}", ("out", "eta", "gsbm", "gdnn"), (out, eta, s.grad, d.grad))
    for tag, x, options in ce_cases():
        for o in options:
            keep(f"ign_loss_{o}.{tag}", CE_OUTPUTS, ce_run(ops, dev, x, o))
    torch.cuda.synchronize()
    np.savez(path, **arrays)
    print(f"{len(arrays)} arrays -> {path}")


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(Bz.files))
    for k in sorted(set(A.files) & set(Bz.files)):
        x, y = A[k], Bz[k]
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            bad.append(k)
    print(f"{len(A.files)} / {len(Bz.files)} arrays, {len(bad)} differ" + (": " + ", ".join(bad[:20]) if bad else " (bitwise equal)"))
    return 1 if bad else 0


def time_entries(path, runs, launches=200, B=256):
    """ms per launch of the three CE entry points at the benchmark's shape (B 256, 3 classes: thread per row) and at 39 classes (wave
    per row): events around `launches` back-to-back launches, `runs` times each, every run kept."""
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    L, st, dev = _lib.lib(), _lib.stream(), torch.device("cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    res = {}
    for N in (3, 39):
        x = {k: v.to(dev) for k, v in ce_inputs(B, N).items()}
        out, gs, gd = (torch.empty(B, N, device=dev) for _ in range(3))
        eta, loss3, reg = torch.empty(B, device=dev), torch.empty(3, device=dev), torch.tensor([CE_REG], device=dev)
        tail = (p(reg), p(out), p(eta), p(loss3), p(gs), p(gd), B, N, CE_BETA)
        calls = {"ign_loss_fwd_bwd_reg": lambda: L.ign_loss_fwd_bwd_reg(p(x["s"]), p(x["d"]), p(x["ya"]), *tail, st),
                 "ign_loss_w_fwd_bwd_reg": lambda: L.ign_loss_w_fwd_bwd_reg(p(x["s"]), p(x["d"]), p(x["ya"]), p(x["w"]), *tail, 0.1, st),
                 "ign_loss_mix_fwd_bwd_reg": lambda: L.ign_loss_mix_fwd_bwd_reg(p(x["s"]), p(x["d"]), p(x["ya"]), p(x["yb"]), p(x["lam"]),
                                                                              p(x["w"]), *tail, 0.1, st)}
        for name, fn in calls.items():
            ms = []
            for _ in range(runs):
                for _ in range(20):
                    assert fn() == 0, name
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(launches):
                    fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b) / launches)
            res[f"{name}.n{N}_b{B}"] = ms
            print(f"{name} N={N} B={B}: {ms}", flush=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, metavar="NPZ", default=None)
    ap.add_argument("--digest", metavar="JSON", default=None)
    ap.add_argument("--time", metavar="JSON", default=None)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if a.digest:
        digest(a.digest)
    if a.time:
        time_entries(a.time, a.runs)
    if a.out or not (a.digest or a.time):
        dump(a.out or "loss_tail.npz")


if __name__ == "__main__":
    main()
