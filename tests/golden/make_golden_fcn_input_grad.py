"""Golden fixture for the gradient w.r.t. the INPUT series through the gated mixture (SBM + FCN expert), from the reference's autograd.

Run (CPU only, seconds):   python tests/golden/make_golden_fcn_input_grad.py

Imports the reference exactly as make_golden.py does (its shims are reused by import) and writes arrays only:
  ign_fcn_input_grad.npz   the reference InterpGN (FCN expert) at B=3 T=60 C=4, 3 classes, with non-trivial BatchNorm running
                           statistics (three train-mode forwards on seeded data before the state is taken):
                             sd.*                     the state_dict every recorded pass starts from
                             x                        (B,T,C)
                             eval.* / train.*         out, eta, dnn_preds, grad_x of out.sum(), grad_x_dnn of dnn_preds.sum()
                                                      with running statistics (eval) resp. batch statistics (train)
The two wide convolution weights (blocks 2 and 3, 262 144 of the model's 270 000 numbers) are rounded to bf16-representable
float32 values BEFORE anything is computed: random mantissas do not compress, and with them the file would not stay below the
1 MiB a committed file may have.  The stored state is exactly the state the reference computed with.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402


def _passes(m, x, train):
    m.train(train)
    xg = x.clone().requires_grad_(True)
    out, info = m(xg, torch.ones(x.shape[0], x.shape[1]), None, None)
    gx, = torch.autograd.grad(out.sum(), xg, retain_graph=True)
    gd, = torch.autograd.grad(info.dnn_preds.sum(), xg)
    tag = "train." if train else "eval."
    return {tag + "out": MG.npy(out), tag + "eta": MG.npy(info.eta), tag + "dnn_preds": MG.npy(info.dnn_preds),
            tag + "grad_x": MG.npy(gx), tag + "grad_x_dnn": MG.npy(gd)}


def case_ign_fcn_input_grad(R):
    I = R["InterpGN"]
    B, T, C, N = 3, 60, 4, 3
    c = MG.cfg(enc_in=C, seq_len=T, num_class=N, c_out=N, dec_in=C)
    torch.manual_seed(5)
    m = I.InterpGN(c)
    with torch.no_grad():
        for blk in (m.deep_model.block2, m.deep_model.block3):
            blk[0].weight.copy_(blk[0].weight.bfloat16().float())
    g = torch.Generator().manual_seed(313)
    m.train()
    with torch.no_grad():
        for _ in range(3):
            m(torch.randn(8, T, C, generator=g) * 1.5 + 0.3, torch.ones(8, T), None, None)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = torch.randn(B, T, C, generator=g) * 2.0 + 0.5
    out = {"x": MG.npy(x)}
    out.update({"sd." + k: MG.npy(v) for k, v in sd.items()})
    out.update(_passes(m, x, train=False))
    m.load_state_dict(sd)
    out.update(_passes(m, x, train=True))
    MG.save("ign_fcn_input_grad", **out)


if __name__ == "__main__":
    case_ign_fcn_input_grad(MG.import_reference())
