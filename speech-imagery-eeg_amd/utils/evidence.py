"""Evidence maps: a class logit laid out over time and electrodes, in closed form.

``utils.saliency`` answers "how much does the logit move if this sample moves" (a gradient).  This module answers "how much of the
logit comes from here": for a linear-head shapelet expert and a GAP + Linear FCN the shares exist exactly and sum to the logit the
model predicted with (completeness), which a gradient cannot offer.  It is the content of the reference's "local" explanation
(IGN/utils/shapelet_util.py:104-155: ``rule * p``, class weight times shapelet activation, painted onto the series at each
shapelet's match position), computed on the device from what the forward already produced:

  sbm   (B,T,C)  feature f = col0_g + k*C + c matched the window [t[b,f]*stride_g, t[b,f]*stride_g + L_g) on electrode c; its share
                 W[n_b,f] * p[b,f] of the logit is spread evenly over that window (ops.shapelet_evidence);
  dnn   (B,T)    cam[b,t] = (1/Tl) sum_c Wfc[n_b,c] relu(bn(y3))[b,t,c] (ops.fcn_cam), each spread evenly over the R = k1+k2+k3-2
                 input samples block 3's step t saw (ops.cam_spread);
  remainder (B,) the FCN head's bias.
With explain="gated" the model's own gate value eta_b (gating_value applied as in Experiment.test) is taken as a per-sample mixing
weight: the maps are eta_b * sbm, (1 - eta_b) * dnn and the remainder (1 - eta_b) * bias.

It works for every distance (L1, MSE, cosine, pearson), both gates (RBF, LTS) and under --mask_padding -- the combinations
input_saliency must refuse included -- because it reads p and t only.  The bilinear and attention heads are refused: they are not
additive in p.  There is no CPU path for the maps; ``evidence_rule`` / ``cam_spread_rule`` are the float32 restatement of
csrc/ign_evidence.h in numpy, which the kernels equal bit for bit.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from utils.explain import EXPLAIN, explained, require_linear_head, resolve_target, session


@dataclass
class Evidence:
    """Fields that do not apply to the chosen ``explain`` are None.  sbm.sum((1,2)) + dnn.sum(1) + remainder == logit up to fp32
    summation error."""
    sbm: Optional[torch.Tensor] = None          # (B,T,C) shapelet-expert map, scaled by eta under "gated"
    dnn: Optional[torch.Tensor] = None          # (B,T)   FCN map on the input axis, scaled by 1 - eta under "gated"
    cam: Optional[torch.Tensor] = None          # (B,Tl)  FCN map on block 3's axis, scaled likewise
    eta: Optional[torch.Tensor] = None          # (B,)    gate value ("gated")
    remainder: Optional[torch.Tensor] = None    # (B,)    the bias share
    logit: Optional[torch.Tensor] = None        # (B,)    the explained logit of the target class, from the model's own forward
    target: Optional[torch.Tensor] = None       # (B,)    long: class explained
    contrib: Optional[torch.Tensor] = None      # (B,F)   W[n_b,:] * p: the reference's "local" ranking key (argsort(-contrib) = s_idx)


def evidence_rule(p, t, W, target, Ks, Ls, strides, C, T, scale=None):
    """numpy float32 restatement of ign_shapelet_evidence_bank (csrc/ign_evidence.h) -> (B,T,C) float32.
    v = fl(fl(W[n_b,f] * p[b,f]) * fl(1/L_g)) is added at every sample of the feature's window, g ascending then k ascending from
    0.0f, one fp32 rounding per operation; t outside [0, Tw_g) and a target outside [0, N) contribute nothing; `scale` (B,)
    multiplies once at the end."""
    p, W = np.asarray(p, np.float32), np.asarray(W, np.float32)
    t, target = np.asarray(t, np.int64), np.asarray(target, np.int64)
    B, N = p.shape[0], W.shape[0]
    tgt_ok = (target >= 0) & (target < N)
    Wn = W[np.where(tgt_ok, target, 0)]                                    # (B,ld)
    out = np.zeros((B, T, C), np.float32)
    s = np.arange(T, dtype=np.int64)[None, :, None]
    col0 = 0
    for K, L, stride in zip(Ks, Ls, strides):
        invL = np.float32(1.0) / np.float32(L)
        Tw = (T - L) // stride + 1
        for k in range(K):
            cols = slice(col0 + k * C, col0 + (k + 1) * C)
            v = (Wn[:, cols] * p[:, cols]) * invL                          # two float32 roundings
            tt = t[:, cols]
            ok = (tt >= 0) & (tt < Tw) & tgt_ok[:, None]
            start = np.where(ok, tt * stride, 0)[:, None, :]
            ln = np.where(ok, L, 0)[:, None, :]
            cover = (s >= start) & (s < start + ln)
            out = out + np.where(cover, v[:, None, :], np.float32(0.0))
        col0 += K * C
    if scale is not None:
        out = out * np.asarray(scale, np.float32)[:, None, None]
    return out


def cam_spread_rule(cam, R):
    """numpy float32 restatement of ign_cam_spread -> (B, Tl + R - 1): out[b,s] = fl(fl(1/R) * sum_{t=max(0,s-R+1)}^{min(s,Tl-1)}
    cam[b,t]), t ascending from 0.0f."""
    cam = np.asarray(cam, np.float32)
    B, Tl = cam.shape
    T = Tl + R - 1
    invR = np.float32(1.0) / np.float32(R)
    out = np.zeros((B, T), np.float32)
    for s in range(T):
        acc = np.zeros(B, np.float32)
        for tt in range(max(0, s - R + 1), min(s, Tl - 1) + 1):
            acc = acc + cam[:, tt]
        out[:, s] = invR * acc
    return out


def _resolve_target(target, logits):
    return resolve_target(target, logits, "evidence_map")


def _sbm_maps(sbm, info, T, idx, scale):
    """(E_sbm (B,T,C), contrib (B,F)) of a linear-head shapelet expert from its forward's ModelInfo."""
    from ign_hip import ops
    W = sbm.output_layer.weight
    if info.t is None:
        raise RuntimeError("evidence_map: the shapelet expert returned no match locations (ModelInfo.t)")
    sbm_map = ops.shapelet_evidence(info.p, info.t, W, idx, [s.n for s in sbm.shapelets], [s.length for s in sbm.shapelets],
                                    [s.stride for s in sbm.shapelets], sbm.num_channel, T, scale=scale)
    return sbm_map, W.detach()[idx] * info.p


def _fcn_maps(fcn, T, idx, scale):
    """(E_dnn (B,T), cam (B,Tl), remainder (B,)) from what the forward that has just run left in fcn.last_block."""
    from ign_hip import ops
    y_last, a, b = fcn.last_block
    if y_last.is_cuda:                       # inside an InterpGN the expert may have run on its side stream
        for ten in (y_last, a, b):
            ten.record_stream(torch.cuda.current_stream(y_last.device))
    cam = ops.fcn_cam(y_last, a, b, fcn.fc.weight, idx, scale=scale)
    dnn = ops.cam_spread(cam, T - y_last.shape[1] + 1)
    bias = fcn.fc.bias.detach()[idx] if fcn.fc.bias is not None else torch.zeros(idx.shape[0], device=cam.device)
    return dnn, cam, bias if scale is None else scale * bias


def evidence_map(model, x, target=None, explain="sbm", gating_value=None, mask=None):
    """-> Evidence, every tensor on x's device: the logit of class target[b] of sample b laid out over the input.

    ``model``: a ShapeBottleneckModel, a DistThresholdSBM ('LTS') or an InterpGN; with explain="dnn" also a FullyConvNetwork -- the
    dispatch, and the TypeErrors, of utils.explain.explained.  ``explain``: "sbm" the interpretable expert's logits
    (``ModelInfo.shapelet_preds``), "dnn" the FCN expert's, "gated" the mixture an InterpGN returns, with ``gating_value`` passed to
    its forward as Experiment.test does (where eta snaps to 1 the FCN map and the remainder are exactly zero).  ``x``: (B,T,C)
    float32 on the GPU.  ``target``: an int, a (B,) integer tensor, or None for the arg-max of the explained logits.  ``mask``: the
    loader's (B,T) keep-mask, honoured by a shapelet expert with ``mask_padding`` on (a shapelet longer than a sample has no match
    and paints nothing); the FCN sees the padded batch, as everywhere.

    A head other than ``--sbm_cls linear`` raises ValueError: the bilinear and attention heads are not additive in p, so no share
    per shapelet exists.  The call runs in eval mode under torch.no_grad(), in fp32 with autocast disabled; one forward of the
    explained model, then one launch per map.  Training flags and the FCN expert's ``keep_last`` switch are restored on return; no
    parameter's ``.grad`` is touched."""
    who = "evidence_map"
    if explain not in EXPLAIN:
        raise ValueError(f"{who}: explain must be one of {EXPLAIN}, got {explain!r}")
    scope, sbm, fcn, call = explained(model, explain, who, gating_value)
    require_linear_head(sbm, who)
    if x.dim() != 3:
        raise ValueError(f"{who}: x must be (B,T,C), got {tuple(x.shape)}")
    T = x.shape[1]
    ev = Evidence()
    with session(scope, fcn=fcn, switch="keep_last"):
        logits, info = call(x.detach().float(), mask)
        idx = resolve_target(target, logits, who)
        if explain == "gated":
            ev.eta = info.eta.reshape(-1).float().contiguous()
        if sbm is not None:
            ev.sbm, ev.contrib = _sbm_maps(sbm, info, T, idx, ev.eta)
        if fcn is not None:
            ev.dnn, ev.cam, ev.remainder = _fcn_maps(fcn, T, idx, None if ev.eta is None else 1.0 - ev.eta)
        ev.target = idx
        ev.logit = logits.float().gather(1, idx[:, None]).squeeze(1)
    return ev
