"""Occlusion maps: a model-agnostic attribution that needs a forward pass only.

Hide a window of time on a group of electrodes behind a baseline, run the model, record how far the score of the explained class
falls, and lay the falls back over the cells that were hidden.  It works for every model of the registry -- the bilinear and
attention heads, every distance, every deep expert, EEGCNN and the Transformer baseline -- because nothing but the model's output is
read.  The occluded copies and the gather back are two HIP passes (``ops.occlude``, ``ops.occlusion_spread``;
csrc/ign_occlusion.hip); what they compute is defined here, in numpy, and the kernels equal it bit for bit:

  grid      W = T if window <= 0 else min(window, T);  S = W if stride <= 0 else stride, 1 <= S <= W;  nt = ceil((T - W) / S) + 1
            windows, the same for every sample; window i covers [i*S, min(i*S + W, n_b)), n_b = clamp(len_b, 0, T);
  patch     p = i*G + g: window i on the electrodes c with gid[c] == g; P = nt*G patches;
  occlude   the copy under patch p holds the bits of fill[b,c] where the patch covers (t, c), elsewhere the bits of x[b,t,c];
  drop      D[b,p] = s0[b] - s[b,p], one float32 subtraction of the explained class's score without and with the patch;
  spread    for t < n_b: M[b,t,c] = (sum_i D[b, i*G + gid[c]]) * inv[cnt(t)] over the windows i = max(0, ceil((t-W+1)/S)) ..
            min(nt-1, t // S) that cover t, added in ascending order one float32 add at a time from the first term; cnt(t) is
            their number and inv[k] = float32(1) / float32(k) a table made on the host; for t >= n_b: +0.0.

Every step is covered by at least one and at most ceil(W / S) windows.  There is no CPU path for the maps.
"""
from typing import NamedTuple, Optional

import numpy as np

from utils.explain import EXPLAIN_ALL, explained, lengths_of, mean_fill, resolve_target, session
from utils.explain import model_logits, shapelet_expert  # noqa: F401  (kept importable from here)
from utils.flag_items import FlagItems, parse_spec

MAX_COVER = 64                                          # IGN_OCC_MAX_COVER = ops.OCC_MAX_COVER: most windows over one time step
EXPLAIN = EXPLAIN_ALL[-1:] + EXPLAIN_ALL[:-1]           # "model" first, as the flag's grammar lists it
FILLS = ("mean", "zero")
SCORES = ("logit", "prob")


# --------------------------------------------------------------------------------------------------------- the rule, in numpy
def grid(T, window=0, stride=0):
    """-> (W, S, nt): the window, the stride and the number of windows over T steps.  A stride above the window would leave steps
    uncovered: ValueError."""
    T, window, stride = int(T), int(window), int(stride)
    if T < 1:
        raise ValueError(f"occlusion grid: T = {T}, need at least one time step")
    W = T if window <= 0 else min(window, T)
    S = W if stride <= 0 else stride
    if not 1 <= S <= W:
        raise ValueError(f"occlusion grid: stride {S} above the window {W} would leave time steps uncovered; need 1 <= stride <= window")
    return W, S, -(-(T - W) // S) + 1


def cover_range(T, W, S, nt):
    """-> (lo (T,), hi (T,)) int64: the windows lo[t] .. hi[t] cover step t."""
    t = np.arange(T, dtype=np.int64)
    lo = np.maximum(0, -(-(t - W + 1) // S))
    hi = np.minimum(nt - 1, t // S)
    return lo, hi


def _lengths(B, T, lengths):
    return np.full(B, T, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, T)


def _gid(gid, groups, C):
    gid, groups = np.asarray(gid), int(groups)
    if gid.shape != (C,) or gid.dtype.kind not in "iu" or groups < 1 or (gid < 0).any() or (gid >= groups).any():
        raise ValueError(f"occlusion: gid must be {C} integers in [0, groups) with groups = {groups} >= 1")
    return gid.astype(np.int64), groups


def occlude_rule(x, p0, count, gid, groups, window, stride, fill=None, lengths=None):
    """x (B,T,C) float32 -> float32 (B*count, T, C): row b*count + q is sample b under patch p0 + q -- the bits of fill[b,c] (0.0f
    without `fill`) where gid[c] == g(p) and i(p)*S <= t < min(i(p)*S + W, n_b), elsewhere the bits of x.  A patch beyond the sample's
    length, or of a group with no electrode, is an exact copy."""
    x = np.ascontiguousarray(x, np.float32)
    B, T, C = x.shape
    W, S, nt = grid(T, window, stride)
    gid, G = _gid(gid, groups, C)
    p0, count = int(p0), int(count)
    if p0 < 0 or count < 1 or p0 + count > nt * G:
        raise ValueError(f"occlude_rule: patches {p0} .. {p0 + count - 1} outside [0, {nt * G})")
    n = _lengths(B, T, lengths)
    p = p0 + np.arange(count, dtype=np.int64)
    lo = (p // G) * S                                                     # (count,)
    hi = np.minimum(lo[None, :] + W, n[:, None])                          # (B, count)
    t = np.arange(T, dtype=np.int64)
    time = (t[None, None, :] >= lo[None, :, None]) & (t[None, None, :] < hi[:, :, None])         # (B, count, T)
    elec = gid[None, :] == (p % G)[:, None]                               # (count, C)
    put = time[:, :, :, None] & elec[None, :, None, :]
    f = np.zeros((B, C), np.float32) if fill is None else np.ascontiguousarray(fill, np.float32)
    out = np.broadcast_to(x.view(np.uint32)[:, None], (B, count, T, C)).copy()                  # on integer views: a NaN keeps its bits
    out[put] = np.broadcast_to(f.view(np.uint32)[:, None, None, :], (B, count, T, C))[put]
    return out.reshape(B * count, T, C).view(np.float32)


def inv_table(cover):
    """float32 (cover + 1,): inv[k] = float32(1) / float32(k), inv[0] = 0 (never read)."""
    inv = np.zeros(int(cover) + 1, np.float32)
    inv[1:] = np.float32(1.0) / np.arange(1, int(cover) + 1, dtype=np.float32)
    return inv


def spread_rule(drop, gid, groups, window, stride, T, lengths=None):
    """drop (B, nt*G) float32 -> float32 (B,T,C): the drops laid back over the cells that were hidden (see the module docstring)."""
    D = np.ascontiguousarray(drop, np.float32)
    W, S, nt = grid(T, window, stride)
    gid, G = _gid(gid, groups, len(np.asarray(gid)))
    B = D.shape[0]
    if D.shape != (B, nt * G):
        raise ValueError(f"spread_rule: drop must be ({B}, {nt * G}), got {D.shape}")
    n = _lengths(B, T, lengths)
    lo, hi = cover_range(T, W, S, nt)
    cnt = hi - lo + 1
    Dg = D.reshape(B, nt, G)[:, :, gid]                                   # (B, nt, C): the drops of each electrode's group
    acc = Dg[:, lo, :].copy()                                             # the first term
    for k in range(1, int(cnt.max())):
        more = (lo + k <= hi)[None, :, None]
        acc = np.where(more, acc + Dg[:, np.minimum(lo + k, nt - 1), :], acc).astype(np.float32)      # one float32 add per term
    out = (acc * inv_table(-(-W // S))[cnt][None, :, None]).astype(np.float32)
    out[np.arange(T)[None, :] >= n[:, None]] = np.float32(0.0)
    return out


def resolve_groups(groups, C):
    """``"all"`` (one group: time-only occlusion), ``"each"`` (a group per electrode), an int array of shape (C,) or the path of a
    ``.npy`` file holding one -> (gid int32 (C,), G).  G = max(gid) + 1; a group id without an electrode is legal (its patches are
    exact copies and their drops are spread nowhere).  Scalp regions are such an array; so are the band blocks of
    ``--eeg_preprocess bank=...``: ``[utils.eeg_filter.bank_channel(res, c)[0] for c in range(C)]``."""
    if isinstance(groups, str):
        if groups == "all":
            return np.zeros(C, np.int32), 1
        if groups == "each":
            return np.arange(C, dtype=np.int32), C
        if not groups.endswith(".npy"):
            raise ValueError(f"occlusion: groups must be all, each, an integer array or a .npy path, got {groups!r}")
        groups = np.load(groups)
    gid = np.asarray(groups.cpu() if hasattr(groups, "cpu") else groups)
    if gid.shape != (C,) or gid.dtype.kind not in "iu" or (gid < 0).any():
        raise ValueError(f"occlusion: groups must hold {C} non-negative integers, one group per electrode, got {gid.dtype} {gid.shape}")
    return np.ascontiguousarray(gid, dtype=np.int32), int(gid.max()) + 1


# --------------------------------------------------------------------------------------------------------- the flag
class OccSpec(NamedTuple):
    """The parsed ``--occlusion`` flag; the field names are keyword arguments of ``occlusion_map``."""
    explain: str
    window: int = 0
    stride: int = 0
    groups: str = "all"
    fill: str = "mean"
    score: str = "logit"
    rows: int = 256


_GRAMMAR = ("none | explain=model|sbm|gated|dnn[,window=W][,stride=S][,groups=all|each|PATH.npy][,fill=mean|zero][,score=logit|prob]"
            "[,rows=R]")
_ITEMS = FlagItems("--occlusion", _GRAMMAR, ("explain", "window", "stride", "groups", "fill", "score", "rows"))


def check_grid_spec(window, stride, groups, who):
    """What every caller refuses about the grid before it knows T: negative numbers, a stride above the window, a groups word."""
    for what, v in (("window", window), ("stride", stride)):
        if isinstance(v, bool) or int(v) != v or int(v) < 0:
            raise ValueError(f"{who}: {what} must be a non-negative integer (0: {'the whole series' if what == 'window' else 'the window'}), "
                             f"got {v!r}")
    if int(window) > 0 and int(stride) > int(window):
        raise ValueError(f"{who}: stride {stride} above the window {window} would leave time steps uncovered")
    if isinstance(groups, str) and groups not in ("all", "each") and not groups.endswith(".npy"):
        raise ValueError(f"{who}: groups must be all, each or the path of a .npy file, got {groups!r}")


def check_spec(explain, window=0, stride=0, groups="all", fill="mean", score="logit", rows=256, who="--occlusion"):
    """The domain of ``occlusion_map`` (what it refuses with ValueError)."""
    if explain not in EXPLAIN:
        raise ValueError(f"{who}: explain must be one of {EXPLAIN}, got {explain!r}")
    check_grid_spec(window, stride, groups, who)
    for what, v, allowed in (("fill", fill, FILLS), ("score", score, SCORES)):
        if v not in allowed:
            raise ValueError(f"{who}: {what} must be one of {allowed}, got {v!r}")
    if isinstance(rows, bool) or int(rows) != rows or int(rows) < 1:
        raise ValueError(f"{who}: rows must be a positive integer (occluded copies per forward), got {rows!r}")


def parse_occlusion(spec):
    """``none`` / ``''`` / None -> None (the flag is off), or ``explain=model,window=50,stride=25,groups=each,fill=mean,score=logit,
    rows=256`` (``explain`` is required, the rest in any order) -> OccSpec.  Unknown or repeated keys, a missing ``explain`` and
    values outside the domain raise ValueError."""
    return parse_spec(_ITEMS, spec, OccSpec, check_spec, "explain=model|sbm|gated|dnn", integers=("window", "stride", "rows"))


# --------------------------------------------------------------------------------------------------------- the map
class Occlusion(NamedTuple):
    """``map`` (B,T,C): the mean drop of the explained class's score over the patches that hid each cell; ``drop`` (B,P) per patch
    p = i*G + g; ``target`` (B,) the explained class; ``base`` (B,) its unperturbed score."""
    map: Optional[object] = None
    drop: Optional[object] = None
    target: Optional[object] = None
    base: Optional[object] = None


def occlusion_map(model, x, mask=None, target=None, explain="model", window=0, stride=0, groups="all", fill="mean", score="logit",
                  rows=256, gating_value=None):
    """-> Occlusion, every tensor on x's device.

    ``explain``: "model" runs the whole model as Experiment.test calls it (any model of the registry: SBM / LTS / InterpGN with any
    head, distance and deep expert, EEGCNN, the DNN baselines); "sbm" | "gated" | "dnn" explain the shapelet expert, the gated
    mixture and the FCN expert (utils.explain.explained, with its TypeErrors) -- but every head and every distance is served, because
    nothing but the output is read.  ``window`` / ``stride``: the time grid (0: the whole series / the window); ``groups``: "all"
    (time-only occlusion, the map is constant across electrodes), "each" (a group per electrode; with ``window=0`` pure electrode
    occlusion), an int array (C,) or a ``.npy`` path (scalp regions, the band blocks of a filter bank).  ``fill``: "mean" replaces a
    hidden cell by its electrode's mean over the sample's own length, "zero" by 0.  ``score``: the explained class's "logit" or
    soft-max "prob".  ``target`` (an int, a (B,) tensor, None: the predicted class) is resolved once, from the unperturbed forward.
    With ``mask_padding`` on in the model's shapelet expert the lengths come from ``mask`` and occlusion stays inside them; else the
    padded batch is occluded whole, which is how the model sees it.

    One unperturbed forward, then per chunk of ``max(1, rows // B)`` patches one ops.occlude launch and one forward on B * chunk
    rows (``mask`` repeated row-wise), then one ops.occlusion_spread launch.  Eval mode, no_grad, fp32 with autocast disabled; every
    module's training flag is restored on return."""
    import torch
    from ign_hip import ops
    who = "occlusion_map"
    check_spec(explain, window, stride, groups, fill, score, rows, who=who)
    scope, sbm, _, call = explained(model, explain, who, gating_value)
    if x.dim() != 3:
        raise ValueError(f"{who}: x must be (B,T,C), got {tuple(x.shape)}")
    B, T, C = x.shape
    W, S, nt = grid(T, window, stride)
    if -(-W // S) > MAX_COVER:
        raise ValueError(f"{who}: window {W} / stride {S} put {-(-W // S)} windows over a time step, more than {MAX_COVER}")
    gid, G = resolve_groups(groups, C)
    P = nt * G

    def pick(logits, idx):
        s = torch.softmax(logits, dim=1) if score == "prob" else logits
        return s.gather(1, idx[:, None]).squeeze(1)

    with session(scope):
        xf = x.detach().float().contiguous()
        logits0 = call(xf, mask)[0].float()
        idx = resolve_target(target, logits0, who)              # fixed before anything is occluded
        base = pick(logits0, idx)
        lengths = lengths_of(sbm, mask, T)
        fill_bc = mean_fill(xf, lengths) if fill == "mean" else None
        if B == 0:
            return Occlusion(map=xf.new_zeros(0, T, C), drop=xf.new_zeros(0, P), target=idx, base=base)
        chunk = max(1, int(rows) // B)
        drops = []
        for p0 in range(0, P, chunk):
            n = min(chunk, P - p0)
            xo = ops.occlude(xf, p0, n, gid, G, window, stride, fill=fill_bc, lengths=lengths)
            logits = call(xo, None if mask is None else mask.repeat_interleave(n, dim=0))[0].float()
            drops.append(base[:, None] - pick(logits, idx.repeat_interleave(n)).view(B, n))
        drop = torch.cat(drops, dim=1).contiguous()
        out = ops.occlusion_spread(drop, gid, G, window, stride, T, lengths=lengths)
    return Occlusion(map=out, drop=drop, target=idx, base=base)


def to_arrays(occ, spec, T, C):
    """What occlusion.npz holds: the maps, the per-patch drops, the explained class and its score, the electrode groups and the grid."""
    W, S, nt = grid(T, spec.window, spec.stride)
    gid, G = resolve_groups(spec.groups, C)
    return dict(map=occ.map.float().cpu().numpy(), drop=occ.drop.float().cpu().numpy(), target=occ.target.cpu().numpy(),
                base=occ.base.float().cpu().numpy(), gid=gid, window=np.int64(W), stride=np.int64(S), windows=np.int64(nt),
                groups=np.int64(G))
