"""Per-sample input saliency of the shapelet expert: the gradient of one class logit w.r.t. the input series.

Complements the match locations in ``ModelInfo.t``: those say WHERE each shapelet matched, this says how much every
(time, channel) sample moves the chosen logit.  The gradient runs through the HIP input-gradient pass of the shapelet bank
(ign_shapelet_bwd_input) and the instance-norm backward (ign_instnorm_bwd); there is no CPU path.
"""
import torch

from models.InterpGN import InterpGN
from models.Shapelet import ShapeBottleneckModel


def _interpretable_expert(model):
    if isinstance(model, InterpGN):
        return model.sbm
    if isinstance(model, ShapeBottleneckModel):
        return model
    raise TypeError(f"input_saliency explains a shapelet expert (SBM, LTS or the SBM inside InterpGN), not {type(model).__name__}")


def input_saliency(model, x, target=None):
    """-> (B,T,C) tensor on x's device: d logit[b, target_b] / d x[b] for every sample b.

    ``model``: a ShapeBottleneckModel, a DistThresholdSBM ('LTS') or an InterpGN.  For an InterpGN the INTERPRETABLE expert is
    explained -- ``model.sbm``, i.e. the logits ``ModelInfo.shapelet_preds`` -- not the gated mixture: the deep expert (FCN and
    the others) has no input gradient and keeps raising if asked for one.
    ``x``: (B,T,C) float32 batch on the GPU in the loader's layout.  ``target``: an int (one class for the whole batch), a (B,)
    integer tensor, or None for each sample's predicted class (arg-max of the expert's logits).
    L1 ('euclidean') and MSE distances only; cosine / pearson raise IgnError.

    The model is evaluated in eval mode (no dropout) with its parameters frozen for the duration of the call, so the backward
    runs the input-gradient kernels only -- no weight or threshold gradient is computed -- and no parameter's ``.grad`` is
    touched.  Every module's training flag and every ``requires_grad`` flag is restored on return.
    """
    expert = _interpretable_expert(model)
    if x.dim() != 3:
        raise ValueError(f"input_saliency: x must be (B,T,C), got {tuple(x.shape)}")
    frozen = [p for p in expert.parameters() if p.requires_grad]
    modes = [(mod, mod.training) for mod in expert.modules()]          # per module: mixed train / eval set-ups come back as they were
    xg = x.detach().clone().requires_grad_(True)
    try:
        expert.eval()
        for p in frozen:
            p.requires_grad_(False)
        with torch.enable_grad():
            logits, _ = expert(xg)
            B = logits.shape[0]
            if target is None:
                idx = logits.detach().argmax(dim=1)
            elif torch.is_tensor(target):
                idx = target.to(device=logits.device, dtype=torch.long).reshape(-1)
                if idx.numel() != B:
                    raise ValueError(f"input_saliency: target has {idx.numel()} entries for a batch of {B}")
            else:
                idx = torch.full((B,), int(target), device=logits.device, dtype=torch.long)
            if bool(((idx < 0) | (idx >= logits.shape[1])).any()):
                raise ValueError(f"input_saliency: target outside [0, {logits.shape[1]})")
            # samples are independent (instance norm and the bank act per sample), so the gradient of the sum of the selected
            # logits is, row by row, the gradient of each sample's own logit
            picked = logits.gather(1, idx[:, None]).sum()
            grad, = torch.autograd.grad(picked, xg)
    finally:
        for p in frozen:
            p.requires_grad_(True)
        for mod, flag in modes:
            mod.training = flag
    return grad
