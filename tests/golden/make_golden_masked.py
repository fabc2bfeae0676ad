"""Golden fixture for --mask_padding: the reference's ShapeBottleneckModel run on TRUNCATED samples, one at a time.

Run (CPU only, seconds):   python tests/golden/make_golden_masked.py

Imports the reference exactly as make_golden.py does (its shims are reused by import) and writes arrays only:
  sbm_masked.npz   shape A of tests/test_gpu_mask_padding.py (seed 0: x = randn(6, 96, 3), w_0 = randn(3, 3, 8), w_1 = randn(2, 3, 40)
                   in float64, cast to fp32; lengths [96, 40, 39, 8, 7, 57]), restricted to the samples with n_b >= 40 (every group
                   has a window there, so the reference runs as it is): `x` (3,96,3) zero-padded, `lengths` (3), `sd.*` of the model
                   (groups K = (3, 2), L = (8, 40), linear head), `r` (3, F), and per sample the reference's `p`, `d` (3, F) of
                   m(x[b:b+1, :n_b]) and `grad.*` = the shapelet gradients of sum_b sum(r[b] * p_b).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

SEED, B, T, C = 0, 6, 96, 3
KS, LS, FRACS = (3, 2), (8, 40), (0.08, 0.41)          # ceil(0.08 * 96) = 8, ceil(0.41 * 96) = 40
LENGTHS = [96, 40, 39, 8, 7, 57]


def case_sbm_masked(R):
    S = R["Shapelet"]
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(B, T, C, generator=g, dtype=torch.float64)
    ws = [torch.randn(K, C, L, generator=g, dtype=torch.float64) for K, L in zip(KS, LS)]
    keep = [b for b, n in enumerate(LENGTHS) if n >= max(LS)]
    lengths = [LENGTHS[b] for b in keep]
    x = x[keep].float()
    for i, n in enumerate(lengths):
        x[i, n:] = 0.0
    torch.manual_seed(5)
    m = S.ShapeBottleneckModel(configs=MG.cfg(enc_in=C, seq_len=T, num_class=4, c_out=4, dec_in=C), num_shapelet=list(KS),
                               shapelet_len=list(FRACS))
    assert [s.weights.shape for s in m.shapelets] == [w.shape for w in ws]
    with torch.no_grad():
        for s, w in zip(m.shapelets, ws):
            s.weights.copy_(w.float())
    m.eval()
    F_ = sum(KS) * C
    r = torch.randn(len(keep), F_, generator=g, dtype=torch.float64).float()
    ps, ds, loss = [], [], 0.0
    for i, n in enumerate(lengths):
        _, info = m(x[i:i + 1, :n])
        ps.append(info.p)
        ds.append(info.d)
        loss = loss + (info.p * r[i:i + 1]).sum()
    loss.backward()
    out = dict(x=MG.npy(x), lengths=np.asarray(lengths, dtype=np.int32), r=MG.npy(r), p=MG.npy(torch.cat(ps)), d=MG.npy(torch.cat(ds)))
    out.update(MG.sd_np(m))
    out.update({f"grad.shapelets.{i}.weights": MG.npy(s.weights.grad) for i, s in enumerate(m.shapelets)})
    MG.save("sbm_masked", **out)


if __name__ == "__main__":
    case_sbm_masked(MG.import_reference())
