"""The explanation host path: what ``explain`` means, and the scaffolding every explainer runs inside.

The four explainers (utils.saliency.input_saliency, utils.evidence.evidence_map, utils.faithfulness.faithfulness_curves,
utils.occlusion.occlusion_map) are their own arithmetic plus three calls into this module:

  ``explained(model, explain, who)``  the dispatch -> (scope, sbm, fcn, call), with the TypeErrors;
  ``session(scope, ...)``             eval mode, the grad / no-grad context, the FCN switch -- and everything restored on the way out;
  ``resolve_target(target, logits)``  an int, a (B,) tensor or None -> the (B,) long classes explained.
``require_linear_head``, ``lengths_of`` and ``mean_fill`` serve those that need them.  A fifth explainer makes the same three calls.

``explain``   scope (put in eval mode)  sbm (lengths, head rule)   fcn         call(x, mask) -> (logits, info)
  "sbm"       the shapelet expert       the same                   None        sbm(x, mask)
  "gated"     the InterpGN              model.sbm                  deep_model  model(x, mask, None, None, gating_value=...)
  "dnn"       the FCN expert            None                       the same    (fcn(x), None)
  "model"     the whole model           its shapelet expert / None None        (model_logits(model, x, mask, gating_value), None)

What differs between the explainers on purpose (changing any of it is a change of behaviour, not of this module):

                           input_saliency         evidence_map          faithfulness_curves     occlusion_map
  explain                  EXPLAIN                EXPLAIN               EXPLAIN_ALL             EXPLAIN_ALL
  the forward              its own: scope(x)[0],  call(x, mask)         call(x, mask)           call(x, mask)
                           model(x, gating_value=...)[0], fcn(x): no mask reaches the model
  x                        as given (no cast)     x.float()             x.float()               x.float()
  context                  enable_grad; an        no_grad, autocast     no_grad, autocast       no_grad, autocast
                           ambient autocast stays off                   off                     off
  frozen parameters        yes                    no                    no                      no
  FCN switch               input_grad             keep_last (+ last_block dropped)   none       none
  linear head required     no                     always                unless only occlusion / random are asked for   no
  refusals, in order       explain, dispatch,     explain, dispatch,    spec, dispatch,         spec, dispatch, x.dim(), grid,
                           x.dim()                linear head, x.dim()  linear head, x.dim()    cover, groups
  Experiment passes        no --gating_value      --gating_value        --gating_value          --gating_value

Importing this module needs neither torch nor the models (the flag parsers import it): both are imported inside the functions.
"""
from contextlib import contextmanager
from typing import Callable, NamedTuple, Optional

EXPLAIN = ("sbm", "gated", "dnn")
EXPLAIN_ALL = EXPLAIN + ("model",)                      # "model": the whole model, as Experiment.test calls it


class Explained(NamedTuple):
    scope: object                                       # the module tree that is put in eval mode
    sbm: Optional[object]                               # the shapelet expert that decides the lengths and the linear-head rule
    fcn: Optional[object]                               # the FCN expert
    call: Callable                                      # (x, mask) -> (logits, info)


def shapelet_expert(model):
    """The shapelet expert whose ``mask_padding`` decides whether a padding mask gives lengths: the model itself (SBM / LTS), the
    ``sbm`` of an InterpGN, or None."""
    from models.InterpGN import InterpGN
    from models.Shapelet import ShapeBottleneckModel
    if isinstance(model, InterpGN):
        return model.sbm
    return model if isinstance(model, ShapeBottleneckModel) else None


def model_logits(model, x, mask=None, gating_value=None):
    """The logits of a registry model on a (B,T,C) batch -- the calling convention of Experiment._forward at test time, by the
    model's type: EEGCNN takes the (B,C,T) permuted view and no mask, InterpGN takes ``gating_value``, the deep baselines (--model
    DNN) return bare logits, the others (logits, info)."""
    from models.InterpGN import InterpGN
    from models.eegcnn import EEGCNNTransformer
    if isinstance(model, EEGCNNTransformer):
        out = model(x.permute(0, 2, 1))
    elif isinstance(model, InterpGN):
        out = model(x, mask, None, None, gating_value=gating_value)
    else:
        out = model(x, mask, None, None)
    return out[0] if isinstance(out, tuple) else out


def explained(model, explain, who, gating_value=None):
    """The dispatch of ``explain`` (one of EXPLAIN_ALL; the caller has checked that) -> Explained; `who` names the caller in the
    TypeErrors.  "gated" and "dnn" need the FCN deep expert: the others have no input-gradient or class-activation kernels."""
    from models.FullyConvNet import FullyConvNetwork
    from models.InterpGN import InterpGN
    if explain == "model":
        import torch
        if not isinstance(model, torch.nn.Module):
            raise TypeError(f'{who}(explain="model") needs a torch.nn.Module, not {type(model).__name__}')
        return Explained(model, shapelet_expert(model), None, lambda x, mask: (model_logits(model, x, mask, gating_value), None))
    if explain == "sbm":
        sbm = shapelet_expert(model)
        if sbm is None:
            raise TypeError(f"{who} explains a shapelet expert (SBM, LTS or the SBM inside InterpGN), not {type(model).__name__}")
        return Explained(sbm, sbm, None, lambda x, mask: sbm(x, mask))
    fcn = model.deep_model if isinstance(model, InterpGN) else model if (explain == "dnn" and isinstance(model, FullyConvNetwork)) else None
    if fcn is None:
        want = "an InterpGN" if explain == "gated" else "an InterpGN or a FullyConvNetwork"
        raise TypeError(f'{who}(explain="{explain}") needs {want} with the FCN deep expert, not {type(model).__name__}')
    if not isinstance(fcn, FullyConvNetwork):
        raise TypeError(f'{who}(explain="{explain}"): FCN is the supported deep expert (--dnn_type FCN), not {type(fcn).__name__}')
    if explain == "dnn":
        return Explained(fcn, None, fcn, lambda x, mask: (fcn(x), None))
    return Explained(model, model.sbm, fcn, lambda x, mask: model(x, mask, None, None, gating_value=gating_value))


def resolve_target(target, logits, who):
    """``target`` -- an int (one class for the batch), a (B,) integer tensor or None (the arg-max of `logits` (B,N)) -> (B,) long on
    the logits' device, inside [0, N)."""
    import torch
    B, N = logits.shape
    if target is None:
        return logits.detach().argmax(dim=1)
    if torch.is_tensor(target):
        idx = target.to(device=logits.device, dtype=torch.long).reshape(-1)
        if idx.numel() != B:
            raise ValueError(f"{who}: target has {idx.numel()} entries for a batch of {B}")
    else:
        idx = torch.full((B,), int(target), device=logits.device, dtype=torch.long)
    if bool(((idx < 0) | (idx >= N)).any()):
        raise ValueError(f"{who}: target outside [0, {N})")
    return idx


def require_linear_head(sbm, who):
    """The bilinear and attention heads are not additive in p, so no share per shapelet -- no evidence map -- exists."""
    if sbm is not None and sbm.configs.sbm_cls != 'linear':
        raise ValueError(f"{who}: --sbm_cls {sbm.configs.sbm_cls} is not additive in the shapelet activations p (the logit has "
                         f"products of them), so no share per shapelet exists; evidence maps need the linear head")


@contextmanager
def session(scope, grad=False, freeze=False, fcn=None, switch=None):
    """Run a block with `scope` in eval mode, under torch.enable_grad() (`grad`) or under torch.no_grad() with autocast disabled on
    the device type of `scope`'s parameters.
    `freeze`: the parameters that require a gradient do not for the duration; `fcn`, `switch` ("input_grad" | "keep_last"): that
    switch of the FCN expert is on for the duration ("keep_last": and what it kept, ``last_block``, is dropped afterwards).  On the way
    out -- a normal exit, an exception, a ``return`` from inside the block -- every module's training flag and every requires_grad
    flag is as it was, and the switch is as it was: the instance attribute it was, or no instance attribute."""
    import torch
    modes = [(mod, mod.training) for mod in scope.modules()]           # per module: mixed train / eval set-ups come back as they were
    frozen = [p for p in scope.parameters() if p.requires_grad] if freeze else []
    if switch is None:
        fcn = None
    had, old = (switch in vars(fcn), getattr(fcn, switch)) if fcn is not None else (False, None)
    try:
        scope.eval()
        for p in frozen:
            p.requires_grad_(False)
        if fcn is not None:
            setattr(fcn, switch, True)
        if grad:
            with torch.enable_grad():
                yield
        else:                                                          # fp32 where the model lives (its input lives there too)
            device_type = next((p.device.type for p in scope.parameters()), "cuda")
            with torch.no_grad(), torch.autocast(device_type=device_type, enabled=False):
                yield
    finally:
        for p in frozen:
            p.requires_grad_(True)
        for mod, flag in modes:
            mod.training = flag
        if fcn is not None:
            if switch == "keep_last":
                vars(fcn).pop("last_block", None)
            if had:
                setattr(fcn, switch, old)
            else:
                vars(fcn).pop(switch, None)


def lengths_of(sbm, mask, T):
    """int32 (B,) lengths inside [0, T] from the loader's keep-mask, or None: no shapelet expert, ``mask_padding`` off, or no mask."""
    import torch
    lengths = sbm.padding_lengths((mask,)) if sbm is not None else None
    return None if lengths is None else lengths.clamp(0, T).to(torch.int32).contiguous()


def mean_fill(xf, lengths):
    """(B,C): the mean of every electrode over the sample's own length (`lengths` int (B,) or None: the whole series) -- what
    ``fill="mean"`` puts in a replaced cell, for the faithfulness curves and the occlusion maps alike."""
    import torch
    if lengths is None:
        return xf.mean(1).contiguous()
    keep = (torch.arange(xf.shape[1], device=xf.device)[None, :] < lengths[:, None]).to(xf.dtype)
    return ((xf * keep[:, :, None]).sum(1) / lengths.clamp(min=1).to(xf.dtype)[:, None]).contiguous()
