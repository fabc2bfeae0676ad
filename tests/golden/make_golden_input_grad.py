"""Golden fixtures for the gradient w.r.t. the INPUT series through the shapelet expert, from the reference's autograd.

Run (CPU only, seconds):   python tests/golden/make_golden_input_grad.py

Imports the reference exactly as make_golden.py does (its shims are reused by import) and writes arrays only:
  input_grad_{l1,mse,lts}.npz  one length group, B=3 C=4 T=60 K=3 L=9: xn, w, (thr), eps, r, p and grad_xn of sum(p * r)
                               (mse: the distance of ShapeletDistanceFunc restated with differentiable torch ops, see below)
  sbm_input_grad.npz           ShapeBottleneckModel (instance norm included) with the linear and the bilinear head at
                               B=3 T=60 C=4: per head `<head>.sd.*`, `<head>.x` (B,T,C), `<head>.out` and `<head>.grad_x` of out.sum()
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(MG.HERE)))
from oracle import ign_oracle as O  # noqa: E402


def case_groups(R):
    S = R["Shapelet"]
    B, C, T, K, L = 3, 4, 60, 3, 9
    g = torch.Generator().manual_seed(311)
    xn0 = torch.randn(B, C, T, generator=g)
    r = torch.randn(B, K * C, generator=g)
    for name, lts in (("l1", False), ("lts", True)):
        torch.manual_seed(7)
        cls = S.DistThresholdShapelet if lts else S.Shapelet
        m = cls(dim_data=C, shapelet_len=L, num_shapelet=K, stride=1, eps=0.7, distance_func="euclidean")
        xn = xn0.clone().requires_grad_(True)
        p, dmin = m(xn)
        (p * r).sum().backward()
        out = dict(xn=MG.npy(xn), r=MG.npy(r), w=MG.npy(m.weights), eps=np.float32(0.7), p=MG.npy(p), grad_xn=MG.npy(xn.grad),
                   grad_w=MG.npy(m.weights.grad))
        if lts:
            out.update(thr=MG.npy(m.threshold))
        MG.save(f"input_grad_{name}", **out)
    # MSE: ShapeletDistanceFunc on the raw (B,C,T) tensor, as make_golden.case_shapelet_modes calls it
    torch.manual_seed(7)
    w = torch.normal(0, 1, (K, C, L)).requires_grad_(True)
    xn = xn0.clone().requires_grad_(True)
    # the reference's ShapeletDistanceFunc is a custom autograd Function that returns no gradient for x (its grad_xn is all
    # zeros), so the same mean squared difference is formed with plain torch ops for autograd -- and checked against it
    d = (xn.unfold(2, L, 1).permute(0, 2, 1, 3).unsqueeze(2) - w).pow(2).mean(dim=-1)          # (B,Tw,K,C)
    assert torch.allclose(d, S.ShapeletDistance(xn0, w.detach()), rtol=1e-6, atol=1e-7)
    eps = 0.7
    maxp, _ = O.rbf_straight_through_max(d, eps)          # the gate of Shapelet.py:77-84 as the oracle states it
    (maxp * r).sum().backward()
    MG.save("input_grad_mse", xn=MG.npy(xn), r=MG.npy(r), w=MG.npy(w), eps=np.float32(eps), p=MG.npy(maxp),
            grad_xn=MG.npy(xn.grad), grad_w=MG.npy(w.grad))


def case_sbm(R):
    S = R["Shapelet"]
    B, T, C = 3, 60, 4
    g = torch.Generator().manual_seed(312)
    x0 = torch.randn(B, T, C, generator=g) * 2.0 + 0.5
    out = {}
    for head, nshp in (("linear", 5), ("bilinear", 2)):
        c = MG.cfg(enc_in=C, seq_len=T, num_class=3, c_out=3, dec_in=C, sbm_cls=head)
        torch.manual_seed(3)
        m = S.ShapeBottleneckModel(configs=c, num_shapelet=[nshp] * 4, shapelet_len=[0.1, 0.2, 0.3, 0.5])
        m.eval()
        x = x0.clone().requires_grad_(True)
        logits, _ = m(x)
        logits.sum().backward()
        out.update({f"{head}.x": MG.npy(x), f"{head}.out": MG.npy(logits), f"{head}.grad_x": MG.npy(x.grad),
                    f"{head}.num_shapelet": np.int64(nshp)})
        out.update(MG.sd_np(m, prefix=f"{head}.sd."))
    MG.save("sbm_input_grad", **out)


if __name__ == "__main__":
    R = MG.import_reference()
    case_groups(R)
    case_sbm(R)
