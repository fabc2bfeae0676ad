"""Bits of the loss tail: every output of ops.ign_loss, ops.ign_crps_loss, ops.crps_loss and ops.gini_gate (forward and backward,
gating_value None and 0.3) for fixed seeds at N in {2, 5, 16, 17, 65, 256} x B in {1, 257, 1025}, written to one .npz.  Run it on two
builds on the same machine and compare the files: a change that only moves or restates the kernels leaves every array bitwise
equal.  Uses the public ops functions only.  A measuring script, not a test.

    python tests/diag_loss_tail.py --out tail.npz
    python tests/diag_loss_tail.py --compare a.npz b.npz        (no device needed; exit status 1 when an array differs)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

NS, BS = (2, 5, 16, 17, 65, 256), (1, 257, 1025)      # B = 1025 crosses the 1024-row tiles of the wide CE tail and the CRPS tails


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, metavar="NPZ", default=None)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    dump(a.out or "loss_tail.npz")


if __name__ == "__main__":
    main()
