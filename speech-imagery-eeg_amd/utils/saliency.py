"""Per-sample input saliency: the gradient of one class logit w.r.t. the input series.

Complements the match locations in ``ModelInfo.t``: those say WHERE each shapelet matched, this says how much every
(time, channel) sample moves the chosen logit.  Three things can be explained (``explain``):
  "sbm"    the interpretable expert's logits -- the HIP input-gradient pass of the shapelet bank (ign_shapelet_bwd_input) and the
           instance-norm backward (ign_instnorm_bwd);
  "gated"  the mixture ``eta*sbm + (1-eta)*dnn`` an InterpGN with the FCN expert predicts with, the dependence of eta on the SBM
           logits included -- the gate backward (ign_gate_bwd) feeds both experts, the FCN side ends in the data-gradient GEMM
           into the raw series (ign_clconv_dgrad_input*);
  "dnn"    the FCN expert's logits (``ModelInfo.dnn_preds``) alone.
There is no CPU path.  What ``explain`` dispatches to, and the session the call runs in, are utils/explain.py's.
"""
import torch

from utils.explain import EXPLAIN, explained, resolve_target, session


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
    who = "input_saliency"
    if explain not in EXPLAIN:
        raise ValueError(f"{who}: explain must be one of {EXPLAIN}, got {explain!r}")
    scope, _, fcn, _ = explained(model, explain, who)
    # its own forward, not Explained.call: no mask reaches the model here (utils/explain.py lists what differs between the explainers)
    run = {"sbm": lambda xg: scope(xg)[0], "gated": lambda xg: model(xg, gating_value=gating_value)[0], "dnn": lambda xg: fcn(xg)}[explain]
    if x.dim() != 3:
        raise ValueError(f"{who}: x must be (B,T,C), got {tuple(x.shape)}")
    xg = x.detach().clone().requires_grad_(True)
    with session(scope, grad=True, freeze=True, fcn=fcn, switch="input_grad"):
        logits = run(xg)
        idx = resolve_target(target, logits, who)
        # samples are independent (instance norm and the bank act per sample, BatchNorm uses its running statistics), so the
        # gradient of the sum of the selected logits is, row by row, the gradient of each sample's own logit
        grad, = torch.autograd.grad(logits.gather(1, idx[:, None]).sum(), xg)
    return grad
