"""Golden fixtures for class heads wider than 16 classes (CHISCO's 39 categories), from the reference.

Run (CPU only, under a minute):   python tests/golden/make_golden_many_class.py

Imports the reference exactly as make_golden.py does (its shims are reused by import) and writes arrays only:
  ign_fcn_n39.npz        InterpGN(FCN), 39 classes, B = 8: outputs, ModelInfo, training loss, gradients, gating_value path
  train_step_ign_n39.npz three Adam steps (lr 5e-3) of the same model
To keep each file well under 1 MiB the initial weights are rounded to fp16-representable values before the reference runs
and stored as float16 (exact); gradients / final weights of the large FCN tensors are stored as (norm, fixed sample) with
make_golden.grads_compact's rule.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

N_CLASS = 39


def _model(R):
    c = MG.cfg(num_class=N_CLASS, c_out=N_CLASS)
    torch.manual_seed(0)
    m = R["InterpGN"].InterpGN(c)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.half().float())
    return m


def sd_half(model, prefix):
    """float tensors as float16 (exact after the rounding in _model), the rest as they are"""
    return {prefix + k: (v.half().numpy() if v.is_floating_point() else MG.npy(v)) for k, v in model.state_dict().items()}


def sd_compact(model, prefix):
    out = {}
    for k, v in model.state_dict().items():
        v = v.detach()
        if v.numel() <= 4096:
            out[prefix + k] = MG.npy(v)
        else:
            out[prefix + "norm." + k] = np.float64(v.double().norm().item())
            out[prefix + "sample." + k] = MG.npy(v.flatten()[MG.sample_idx(v.numel())])
    return out


def case_ign_n39(R):
    B = 8
    g = torch.Generator().manual_seed(141)
    x = torch.randn(B, 100, 6, generator=g)
    y = torch.randperm(N_CLASS, generator=g)[:B]
    m = _model(R)
    sd0 = sd_half(m, "sd.")
    m.train()
    out, info = m(x, torch.ones(B, 100), None, None)
    ce = torch.nn.functional.cross_entropy
    loss = ce(out, y) + info.loss.mean() + 1.0 * ce(info.shapelet_preds, y)
    loss.backward()
    arrs = dict(x=MG.npy(x), y=MG.npy(y), out=MG.npy(out), eta=MG.npy(info.eta), shapelet_preds=MG.npy(info.shapelet_preds),
                dnn_preds=MG.npy(info.dnn_preds), p=MG.npy(info.p), model_loss=MG.npy(info.loss), train_loss=MG.npy(loss),
                **MG.grads_compact(m, "grad"))
    m.eval()
    with torch.no_grad():
        out_e, _ = m(x, torch.ones(B, 100), None, None)
        out_g, info_g = m(x, torch.ones(B, 100), None, None, gating_value=0.05)
    arrs.update(eval_out=MG.npy(out_e), gated_out=MG.npy(out_g), gated_eta=MG.npy(info_g.eta))
    MG.save("ign_fcn_n39", **arrs, **sd0)


def case_train_steps_n39(R):
    m = _model(R)
    sd0 = sd_half(m, "sd0.")
    g = torch.Generator().manual_seed(161)
    xs = torch.randn(3, 8, 100, 6, generator=g)
    ys = torch.randint(0, N_CLASS, (3, 8), generator=g)
    ce = torch.nn.functional.cross_entropy

    def step(m, x, y):
        out, info = m(x, torch.ones(8, 100), None, None)
        return ce(out, y) + info.loss.mean() + 1.0 * ce(info.shapelet_preds, y)

    losses = MG._three_steps(m, step, [(xs[i], ys[i]) for i in range(3)])
    MG.save("train_step_ign_n39", xs=MG.npy(xs), ys=MG.npy(ys), losses=losses, **sd0, **sd_compact(m, "sd3."))


if __name__ == "__main__":
    R = MG.import_reference()
    case_ign_n39(R)
    case_train_steps_n39(R)
