"""Faithfulness curves: the deletion / insertion test of an explanation (AOPC, "pixel flipping").

An attribution map says which (time, electrode) cells carry a prediction; this module asks the model whether that is so.  The cells of
every sample are ranked by the map, the top fraction f_j = j / steps is replaced by a baseline (``mode="deletion"``; with
``mode="insertion"`` everything BUT the top fraction is), the model runs again and the score of the explained class is recorded
against the fraction, next to the same curve under a random ranking.  The ranking and the perturbation are two HIP passes
(``ops.rank_threshold``, ``ops.perturb``; csrc/ign_faithfulness.hip); what they compute is defined here, in numpy, and the kernels
equal it bit for bit:

  key(v)    u = bits(v); key = ~u if the sign bit is set, else u | 0x80000000 -- the uint32 of the artifact stage (art_key), a total
            order on bit patterns: -0 sorts below +0, positive NaNs above +inf, nothing is special-cased;
  order     element i precedes i' iff key_i > key_i', or the keys are equal and i < i' (highest score first, ties to the lowest flat
            index i = t*Cs + c);
  threshold (key, index) of the k-th element in that order, k clamped to [0, n_b]; k = 0: (0xffffffff, -1);
  selected  i < n_b and (key_i > thr_key or (key_i == thr_key and i <= thr_idx)): elementwise, exactly min(k, n_b) elements, nested
            for ascending k.

Ties are the normal case -- an evidence map is constant over a matched window and exactly zero elsewhere -- which is why the order is
total.  There is no CPU path for the curves.
"""
from dataclasses import dataclass, field
from typing import NamedTuple, Optional

import numpy as np

from utils.explain import EXPLAIN_ALL, explained, lengths_of, mean_fill, require_linear_head, resolve_target, session
from utils.flag_items import FlagItems, parse_spec

MAX_STEPS = 31                                          # steps + 1 thresholds per sample <= IGN_RANK_MAX_K = ops.RANK_MAX_K
ATTRIBUTIONS = ("evidence", "saliency", "random")       # the default request
ALLOWED_ATTRIBUTIONS = ATTRIBUTIONS + ("occlusion",)    # what may be asked for under explain=sbm|gated|dnn
MODEL_ATTRIBUTIONS = ("occlusion", "random")            # ... and under explain=model: the attributions that need only a forward pass
MODES = ("deletion", "insertion")
FILLS = ("mean", "zero")
UNITS = ("cell", "time")
NO_KEY, NO_IDX = 0xffffffff, -1                         # the threshold of k = 0: nothing is selected


# --------------------------------------------------------------------------------------------------------- the rule, in numpy
def key_of(v):
    """float32 array -> uint32 keys of the same order (the mapping of art_key, csrc/ign_eeg_artifact.hip)."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def valid_counts(B, T, Cs, lengths=None):
    """n_b (B,) int64: the scores of sample b that take part, clamp(len_b, 0, T) * Cs."""
    if lengths is None:
        return np.full(B, T * Cs, np.int64)
    return np.clip(np.asarray(lengths, np.int64), 0, T) * Cs


def rank_rule(S, k, lengths=None):
    """S (B,T,Cs) float32, k (B,nk) int -> (thr_key (B,nk) uint32, thr_idx (B,nk) int32): key and flat index of the k-th element of
    each sample in the order above, (0xffffffff, -1) for k = 0; k is clamped to [0, n_b]."""
    S = np.asarray(S, np.float32)
    k = np.asarray(k, np.int64)
    B, T, Cs = S.shape
    n = valid_counts(B, T, Cs, lengths)
    thr_key = np.full(k.shape, NO_KEY, np.uint32)
    thr_idx = np.full(k.shape, NO_IDX, np.int32)
    for b in range(B):
        keys = key_of(S[b].reshape(-1)[:n[b]])
        order = np.argsort(~keys, kind="stable")          # descending key; a stable sort leaves equal keys in index order
        for j, kk in enumerate(np.clip(k[b], 0, n[b])):
            if kk > 0:
                thr_key[b, j] = keys[order[kk - 1]]
                thr_idx[b, j] = order[kk - 1]
    return thr_key, thr_idx


def selected_rule(S, thr_key, thr_idx, j, lengths=None):
    """-> (B, T*Cs) bool: the elements of every sample inside the top-k set of column j."""
    S = np.asarray(S, np.float32)
    B, T, Cs = S.shape
    n = valid_counts(B, T, Cs, lengths)
    keys = key_of(S.reshape(B, -1))
    i = np.arange(T * Cs, dtype=np.int64)[None, :]
    tk = np.asarray(thr_key)
    tk = (tk.view(np.uint32) if tk.dtype == np.int32 else tk.astype(np.uint32))[:, j][:, None]     # int32: the bits, as ops returns them
    ti = np.asarray(thr_idx, np.int64)[:, j][:, None]
    return (i < n[:, None]) & ((keys > tk) | ((keys == tk) & (i <= ti)))


def perturb_rule(x, S, thr_key, thr_idx, j, fill=None, insert=False, lengths=None):
    """x (B,T,C) float32 -> float32 (B,T,C): for t < len_b the fill[b,c] (0.0f without `fill`) where the cell is selected XOR
    `insert`, elsewhere -- and for t >= len_b -- the bits of x.  The score of cell (t, c) is S[b,t,c], or S[b,t,0] when Cs == 1."""
    x = np.ascontiguousarray(x, np.float32)
    B, T, C = x.shape
    Cs = np.asarray(S).shape[2]
    if Cs not in (1, C):
        raise ValueError(f"perturb_rule: score has {Cs} columns for {C} electrodes")
    sel = selected_rule(S, thr_key, thr_idx, j, lengths).reshape(B, T, Cs)
    sel = np.broadcast_to(sel, (B, T, C))
    length = np.full(B, T, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, T)
    inside = np.arange(T)[None, :, None] < length[:, None, None]
    f = np.zeros((B, C), np.float32) if fill is None else np.asarray(fill, np.float32)
    put = inside & (sel != bool(insert))
    out = x.view(np.uint32).copy()                         # on integer views: a NaN in x or fill keeps its bits
    out[put] = np.broadcast_to(np.ascontiguousarray(f).view(np.uint32)[:, None, :], (B, T, C))[put]
    return out.view(np.float32)


# --------------------------------------------------------------------------------------------------------- the flag
class FaithSpec(NamedTuple):
    """The parsed ``--faithfulness`` flag; the field names are keyword arguments of ``faithfulness_curves``."""
    explain: str
    attributions: tuple = ATTRIBUTIONS
    steps: int = 10
    mode: str = "deletion"
    fill: str = "mean"
    unit: str = "cell"
    seed: int = 0
    window: int = 0                                     # the grid of the "occlusion" attribution (utils.occlusion.grid)
    stride: int = 0
    groups: str = "all"


_GRAMMAR = ("none | explain=sbm|gated|dnn|model[,attr=evidence+saliency+random+occlusion][,steps=N][,mode=deletion|insertion]"
            "[,fill=mean|zero][,unit=cell|time][,seed=S][,window=W][,stride=S][,groups=all|each|PATH.npy]")
_ITEMS = FlagItems("--faithfulness", _GRAMMAR, ("explain", "attr", "steps", "mode", "fill", "unit", "seed", "window", "stride", "groups"))


def check_spec(explain, attributions, steps, mode, fill, unit, seed=0, window=0, stride=0, groups="all", who="--faithfulness"):
    """The domain of ``faithfulness_curves`` (what it refuses with ValueError)."""
    if explain not in EXPLAIN_ALL:
        raise ValueError(f"{who}: explain must be one of {EXPLAIN_ALL}, got {explain!r}")
    attributions = tuple(attributions)
    allowed = MODEL_ATTRIBUTIONS if explain == "model" else ALLOWED_ATTRIBUTIONS
    if not attributions or len(set(attributions)) != len(attributions) or any(a not in allowed for a in attributions):
        raise ValueError(f"{who}: attributions must be distinct names from {allowed} under explain={explain}, got {attributions!r}")
    if "occlusion" in attributions:
        from utils.occlusion import check_grid_spec
        check_grid_spec(window, stride, groups, who)
    if int(steps) != steps or not 1 <= int(steps) <= MAX_STEPS:
        raise ValueError(f"{who}: steps must be an integer in 1..{MAX_STEPS}, got {steps}")
    for what, v, allowed in (("mode", mode, MODES), ("fill", fill, FILLS), ("unit", unit, UNITS)):
        if v not in allowed:
            raise ValueError(f"{who}: {what} must be one of {allowed}, got {v!r}")
    if int(seed) != seed or not 0 <= int(seed) < 2 ** 63:
        raise ValueError(f"{who}: seed must be an integer in [0, 2^63), got {seed}")


def parse_faithfulness(spec):
    """``none`` / ``''`` / None -> None (the flag is off), or ``explain=sbm,attr=evidence+random,steps=10,mode=deletion,fill=mean,
    unit=cell,seed=0`` (``explain`` is required, the rest in any order) -> FaithSpec.  Unknown or repeated keys, a missing
    ``explain`` and values outside the domain raise ValueError."""
    return parse_spec(_ITEMS, spec, FaithSpec, check_spec, "explain=sbm|gated|dnn|model", integers=("steps", "seed", "window", "stride"),
                      convert={"attr": ("attributions", lambda val: tuple(a.strip() for a in val.split("+")))})


# --------------------------------------------------------------------------------------------------------- the curves
@dataclass
class Faithfulness:
    """Curves of one batch (or, from ``concat``, of a whole loader).  Per attribution name a: ``logit[a]`` / ``prob[a]`` (steps+1, B)
    the target class's logit / soft-max probability at every fraction, ``flip_at[a]`` (B,) the smallest fraction at which the arg-max
    leaves the target (1 if it never does); the summaries ``auc[a]`` (trapezoid of the mean probability over the fractions),
    ``aopc[a]`` (mean over j >= 1 and the samples of logit_0 - logit_j), ``flip[a]`` (mean of flip_at) and, when "random" was asked
    for, ``gap[a]`` = auc[random] - auc[a] for deletion, auc[a] - auc[random] for insertion: positive where the map beats chance."""
    fractions: Optional[object] = None              # (steps+1,) float64 tensor
    target: Optional[object] = None                 # (B,) long
    mode: str = "deletion"
    logit: dict = field(default_factory=dict)
    prob: dict = field(default_factory=dict)
    flip_at: dict = field(default_factory=dict)
    auc: dict = field(default_factory=dict)
    aopc: dict = field(default_factory=dict)
    flip: dict = field(default_factory=dict)
    gap: dict = field(default_factory=dict)


def summarize(f):
    """Fill the summary numbers of a Faithfulness from its per-sample curves -> f."""
    fr = f.fractions.double().cpu()
    f.auc, f.aopc, f.flip, f.gap = {}, {}, {}, {}
    for a in f.logit:
        lg, pr = f.logit[a].double().cpu(), f.prob[a].double().cpu()
        if lg.shape[1] == 0:
            f.auc[a] = f.aopc[a] = f.flip[a] = float("nan")
            continue
        m = pr.mean(1)
        f.auc[a] = float((0.5 * (m[1:] + m[:-1]) * (fr[1:] - fr[:-1])).sum())
        f.aopc[a] = float((lg[:1] - lg[1:]).mean())
        f.flip[a] = float(f.flip_at[a].double().mean())
    if "random" in f.auc:
        sign = 1.0 if f.mode == "deletion" else -1.0
        f.gap = {a: sign * (f.auc["random"] - f.auc[a]) for a in f.auc}
    return f


def concat(parts):
    """Faithfulness objects of consecutive batches -> one over all their samples, on the host, summaries recomputed."""
    import torch
    first = parts[0]
    out = Faithfulness(fractions=first.fractions.cpu(), mode=first.mode, target=torch.cat([p.target.cpu() for p in parts]))
    for a in first.logit:
        out.logit[a] = torch.cat([p.logit[a].cpu() for p in parts], dim=1)
        out.prob[a] = torch.cat([p.prob[a].cpu() for p in parts], dim=1)
        out.flip_at[a] = torch.cat([p.flip_at[a].cpu() for p in parts])
    return summarize(out)


def _scores(name, model, x, mask, idx, explain, gating_value, gen, fill="mean", window=0, stride=0, groups="all"):
    """The score map (B,T,Cs) of one attribution for the classes `idx`."""
    import torch
    if name == "occlusion":
        from utils import occlusion
        return occlusion.occlusion_map(model, x, mask=mask, target=idx, explain=explain, window=window, stride=stride, groups=groups,
                                       fill=fill, gating_value=gating_value).map
    if name == "evidence":
        from utils import evidence
        ev = evidence.evidence_map(model, x, target=idx, explain=explain, gating_value=gating_value, mask=mask)
        if explain == "sbm":
            return ev.sbm
        if explain == "dnn":
            return ev.dnn[..., None]
        return ev.sbm + ev.dnn[..., None] / x.shape[2]
    if name == "saliency":
        from utils import saliency
        return saliency.input_saliency(model, x, target=idx, explain=explain, gating_value=gating_value).abs()
    return torch.rand(x.shape, device=x.device, dtype=torch.float32, generator=gen)


def faithfulness_curves(model, x, mask=None, target=None, explain="sbm", attributions=ATTRIBUTIONS, steps=10, mode="deletion",
                        fill="mean", unit="cell", seed=0, window=0, stride=0, groups="all", gating_value=None):
    """-> Faithfulness, every tensor on x's device: the explained class's logit and probability of every sample with the top
    j / steps of its cells (``unit="cell"``) or time steps (``unit="time"``: the scores are summed over the electrodes) replaced, for
    j = 0 .. steps and every attribution in ``attributions``:

      "evidence"  utils.evidence.evidence_map: the shapelet expert's map ("sbm"), the FCN expert's per-time-step map ("dnn", one
                  score per time step whatever the unit) or, for "gated", sbm + dnn / C per cell;
      "saliency"  |utils.saliency.input_saliency|; what that refuses (cosine / pearson distances) is refused here with its own error,
                  and like it the gradient is taken on the padded batch, without the mask;
      "random"    torch.rand on the device under a generator seeded with ``seed``;
      "occlusion" utils.occlusion.occlusion_map on the grid ``window`` / ``stride`` / ``groups`` with the same ``fill``: the mean fall
                  of the class logit over the patches that hid a cell.  Not in the default request.

    ``model``, ``explain``, ``gating_value``, ``mask`` and the TypeErrors / ValueErrors of the dispatch are evidence_map's, the
    linear-head requirement included -- except that a bilinear or attention head is accepted when nothing but "occlusion" and
    "random" is asked for, which need no additivity.  ``explain="model"`` runs the whole model as Experiment.test calls it (every
    model of the registry: any head, distance and deep expert, EEGCNN, the DNN baselines) and allows those two attributions only.  ``target`` (an int, a (B,) tensor, None: the predicted class) is resolved once, from the
    unperturbed forward, and shared by every attribution.  ``fill="mean"`` replaces a cell by the mean of its electrode over the
    sample's own length, ``"zero"`` by 0.  With ``mask_padding`` on, the lengths come from ``mask``: only a sample's own steps are
    ranked and replaced.  k[b,j] = (j * n_b) // steps cells are replaced at fraction j / steps.

    Per attribution: one ops.rank_threshold launch, then per j one ops.perturb launch and one forward.  Eval mode, no_grad, fp32
    with autocast disabled; every module's training flag is restored on return."""
    import torch
    from ign_hip import ops
    who = "faithfulness_curves"
    check_spec(explain, attributions, steps, mode, fill, unit, seed, window, stride, groups, who=who)
    attributions, steps = tuple(attributions), int(steps)
    scope, sbm, _, call = explained(model, explain, who, gating_value)
    if explain != "model" and not set(attributions) <= set(MODEL_ATTRIBUTIONS):     # "occlusion" and "random" need no additivity
        require_linear_head(sbm, who)
    if x.dim() != 3:
        raise ValueError(f"{who}: x must be (B,T,C), got {tuple(x.shape)}")
    B, T, C = x.shape

    def forward(xb):
        return call(xb, mask)[0].float()

    out = Faithfulness(mode=mode)
    with session(scope):
        xf = x.detach().float().contiguous()
        idx = resolve_target(target, forward(xf), who)          # fixed before anything is perturbed
        lengths = lengths_of(sbm, mask, T)
        fill_bc = mean_fill(xf, lengths) if fill == "mean" else None
        steps_j = torch.arange(steps + 1, device=x.device, dtype=torch.int64)
        gen = torch.Generator(device=x.device).manual_seed(int(seed))
        out.fractions = steps_j.double() / steps
        out.target = idx
        for name in attributions:
            score = _scores(name, model, xf, mask, idx, explain, gating_value, gen, fill, window, stride, groups)
            if unit == "time" and score.shape[2] != 1:
                score = score.sum(2, keepdim=True)
            score = score.detach().float().contiguous()
            n_b = (lengths.long() if lengths is not None else torch.full((B,), T, device=x.device)) * score.shape[2]
            k = ((steps_j[None, :] * n_b[:, None]) // steps).to(torch.int32).contiguous()
            thr_key, thr_idx = ops.rank_threshold(score, k, lengths=lengths)
            lg, pr, am = [], [], []
            for j in range(steps + 1):
                xp = ops.perturb(xf, score, thr_key, thr_idx, j, fill=fill_bc, insert=(mode == "insertion"), lengths=lengths)
                logits = forward(xp)
                lg.append(logits.gather(1, idx[:, None]).squeeze(1))
                pr.append(torch.softmax(logits, dim=1).gather(1, idx[:, None]).squeeze(1))
                am.append(logits.argmax(1) != idx)
            out.logit[name], out.prob[name] = torch.stack(lg), torch.stack(pr)
            left = torch.stack(am)                               # (steps+1, B): the arg-max has left the target
            first = torch.where(left, steps_j[:, None], steps).min(0).values if B else steps_j[:0]
            out.flip_at[name] = first.double() / steps
    return summarize(out)


# --------------------------------------------------------------------------------------------------------- the files of run.py
def to_json(f, spec):
    """What faithfulness.json holds: the spec, the mean curves and the summary numbers."""
    names = list(f.logit)
    doc = dict(spec._asdict(), attributions=list(spec.attributions))
    if "occlusion" not in spec.attributions:                # the grid belongs to that attribution alone
        for key in ("window", "stride", "groups"):
            del doc[key]
    return dict(spec=doc, samples=int(f.target.shape[0]),
                fractions=[float(v) for v in f.fractions],
                mean_logit={a: [float(v) for v in f.logit[a].double().mean(1)] for a in names},
                mean_prob={a: [float(v) for v in f.prob[a].double().mean(1)] for a in names},
                auc=f.auc, aopc=f.aopc, flip=f.flip, gap=f.gap)


def to_arrays(f):
    """What faithfulness.npz holds: the per-sample curves."""
    arrays = dict(fractions=f.fractions.double().cpu().numpy(), target=f.target.cpu().numpy())
    for a in f.logit:
        arrays[f"logit_{a}"] = f.logit[a].float().cpu().numpy()
        arrays[f"prob_{a}"] = f.prob[a].float().cpu().numpy()
        arrays[f"flip_at_{a}"] = f.flip_at[a].double().cpu().numpy()
    return arrays
