"""Per-sample input saliency: the gradient of one class logit w.r.t. the input series.

Complements the match locations in ``ModelInfo.t``: those say WHERE each shapelet matched, this says how much every
(time, channel) sample moves the chosen logit.  Three things can be explained (``explain``):
  "sbm"    the interpretable expert's logits -- the HIP input-gradient pass of the shapelet bank (ign_shapelet_bwd_input) and the
           instance-norm backward (ign_instnorm_bwd);
  "gated"  the mixture ``eta*sbm + (1-eta)*dnn`` an InterpGN with the FCN expert predicts with, the dependence of eta on the SBM
           logits included -- the gate backward (ign_gate_bwd) feeds both experts, the FCN side ends in the data-gradient GEMM
           into the raw series (ign_clconv_dgrad_input*);
  "dnn"    the FCN expert's logits (``ModelInfo.dnn_preds``) alone.
There is no CPU path.
"""
import torch

from models.FullyConvNet import FullyConvNetwork
from models.InterpGN import InterpGN
from models.Shapelet import ShapeBottleneckModel

EXPLAIN = ("sbm", "gated", "dnn")


def _interpretable_expert(model, who="input_saliency"):
    if isinstance(model, InterpGN):
        return model.sbm
    if isinstance(model, ShapeBottleneckModel):
        return model
    raise TypeError(f"{who} explains a shapelet expert (SBM, LTS or the SBM inside InterpGN), not {type(model).__name__}")


def _fcn_expert(model, explain, who="input_saliency"):
    """The FCN expert behind explain="gated" / "dnn"; the other deep experts have no input-gradient (or class-activation) kernels.
    `who`: the caller named in the error (utils.evidence shares the dispatch)."""
    fcn = model.deep_model if isinstance(model, InterpGN) else model if (explain == "dnn" and isinstance(model, FullyConvNetwork)) else None
    if fcn is None:
        want = "an InterpGN" if explain == "gated" else "an InterpGN or a FullyConvNetwork"
        raise TypeError(f'{who}(explain="{explain}") needs {want} with the FCN deep expert, not {type(model).__name__}')
    if not isinstance(fcn, FullyConvNetwork):
        raise TypeError(f'{who}(explain="{explain}"): FCN is the supported deep expert (--dnn_type FCN), '
                        f'not {type(fcn).__name__}')
    return fcn


def input_saliency(model, x, target=None, explain="sbm", gating_value=None):
    """-> (B,T,C) tensor on x's device: d logit[b, target_b] / d x[b] for every sample b.

    ``model``: a ShapeBottleneckModel, a DistThresholdSBM ('LTS') or an InterpGN; with explain="dnn" also a FullyConvNetwork.
    ``explain``: "sbm" (default) explains the INTERPRETABLE expert -- ``model.sbm`` of an InterpGN, i.e. the logits
    ``ModelInfo.shapelet_preds``; "gated" the mixture an InterpGN returns (``gating_value`` is passed to its forward, as
    Experiment.test does: where eta snaps to 1 the FCN contributes exactly zero); "dnn" the FCN expert's logits.  "gated" and
    "dnn" need the FCN deep expert: the others have no input gradient and keep raising if asked for one.
    ``x``: (B,T,C) float32 batch on the GPU in the loader's layout.  ``target``: an int (one class for the whole batch), a (B,)
    integer tensor, or None for each sample's predicted class (arg-max of the explained logits).
    L1 ('euclidean') and MSE distances only; cosine / pearson raise IgnError.

    The explained modules are evaluated in eval mode (no dropout, running BatchNorm statistics) with their parameters frozen for
    the duration of the call, so the backward runs the input-gradient kernels only -- no weight or threshold gradient is computed
    -- and no parameter's ``.grad`` is touched.  Every module's training flag, every ``requires_grad`` flag and the FCN expert's
    ``input_grad`` switch are restored on return; ``x`` is not modified.
    """
    if explain not in EXPLAIN:
        raise ValueError(f"input_saliency: explain must be one of {EXPLAIN}, got {explain!r}")
    fcn = None
    if explain == "sbm":
        scope = _interpretable_expert(model)
        run = lambda xg: scope(xg)[0]
    else:
        fcn = _fcn_expert(model, explain)
        if explain == "gated":
            scope = model
            run = lambda xg: model(xg, gating_value=gating_value)[0]
        else:
            scope = fcn
            run = lambda xg: fcn(xg)
    if x.dim() != 3:
        raise ValueError(f"input_saliency: x must be (B,T,C), got {tuple(x.shape)}")
    frozen = [p for p in scope.parameters() if p.requires_grad]
    modes = [(mod, mod.training) for mod in scope.modules()]           # per module: mixed train / eval set-ups come back as they were
    had_switch = fcn is not None and "input_grad" in vars(fcn)
    switch = fcn.input_grad if fcn is not None else None
    xg = x.detach().clone().requires_grad_(True)
    try:
        scope.eval()
        for p in frozen:
            p.requires_grad_(False)
        if fcn is not None:
            fcn.input_grad = True
        with torch.enable_grad():
            logits = run(xg)
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
            # samples are independent (instance norm and the bank act per sample, BatchNorm uses its running statistics), so the
            # gradient of the sum of the selected logits is, row by row, the gradient of each sample's own logit
            picked = logits.gather(1, idx[:, None]).sum()
            grad, = torch.autograd.grad(picked, xg)
    finally:
        for p in frozen:
            p.requires_grad_(True)
        for mod, flag in modes:
            mod.training = flag
        if fcn is not None:
            if had_switch:
                fcn.input_grad = switch
            else:
                vars(fcn).pop("input_grad", None)
    return grad
