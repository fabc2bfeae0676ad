"""Artifact stage (``--eeg_artifact``): the flag's parser, the resolver against the electrode count, and the rule that
``ign_eeg_artifact_stats_nct`` / ``ign_eeg_artifact_apply_nct`` (``ops.eeg_artifact``) run, stated once in numpy -- what the CPU item
path applies per item and what the tests compare the kernels against.  The stage is the FIRST of the chain: it judges every (b, c) row
of the raw (B, C, T) batch in front of ``--eeg_spatial``, so a bad electrode is rebuilt before anything mixes electrodes, and keeps
layout and shape.  Nothing is dropped: trial rejection would change batch shapes.

Per sample, rows x[c, :] of length T in fp32; med(v) is the LOWER median, the element of rank (n - 1) // 2 of the sorted values:

    m_c = med(x[c]) (+0.0 where that is -0.0);   s_c = med(|x[c] - m_c|)        each difference one fp32 subtraction
    a row with a non-finite sample has no statistics: verdict 3, (m, s) reported as (0, 0)
    ref = med(s_c over the finite rows)
    flat (1):  s_c <= fl(F * ref)       noisy (2):  s_c > fl(N * ref)           an absent key switches its test off
    no good row left in the sample: every bad row gets 4 (unrepaired) and passes through clamped only, a non-finite one as zeros
    good rows with clip=K:  r = fl(fl(K * 1.4826f) * s_c),  lo = fl(m_c - r),  hi = fl(m_c + r),  y = x < lo ? lo : x > hi ? hi : x
    bad row c:  y[c, t] = (sum_j w[c, j] * fl(y[j, t] - m_j)) / (sum_j w[c, j])       j over the good rows, ascending

``flat=0`` (only a row with s_c = 0 is flat) travels as the smallest positive fp32: the kernels read a non-positive key as absent.
w is the (C, C) non-negative matrix of ``neighbors=PATH.npy`` (the diagonal is never read), all ones without the key, and all ones
for a bad row without a good neighbour of positive weight.  The good rows enter about their own medians: a repaired row carries no
amplifier offset, and the recordings' offsets of 2e4 uV stay out of the summation error.  Everything up to and including the clamp is
bit for bit what the device computes; the repair sum is an fmaf chain there and a multiply-add chain here (``repair64=True``: the
sums in float64, unrounded -- the tests' reference).

No torch in this module except where the stage's ``device_fn`` / ``report_pass`` meet the device.
"""
import hashlib
import json
import os
from typing import NamedTuple, Optional

import numpy as np

from utils.flag_items import FlagItems

MAX_ROW = 16384                                     # IGN_EEG_ARTIFACT_MAX_ROW: one row staged in LDS
MAX_CHANNELS = 1024                                 # IGN_EEG_ARTIFACT_MAX_CHANNELS
MAD_TO_SIGMA = np.float32(1.4826)
GOOD, FLAT, NOISY, NONFINITE, UNREPAIRED = 0, 1, 2, 3, 4
CODE_NAMES = ('good', 'flat', 'noisy', 'nonfinite', 'unrepaired')
FILE_NAME = "eeg_artifact.json"


class EEGArtifactSpec(NamedTuple):
    """The parsed ``--eeg_artifact`` flag."""
    clip: Optional[float] = None                    # clamp radius of the good rows in robust standard deviations
    flat: Optional[float] = None                    # a row is flat at s_c <= flat * ref
    noisy: Optional[float] = None                   # a row is noisy at s_c > noisy * ref
    neighbors: Optional[str] = None                 # path of the (C, C) weight matrix
    report: bool = False
    given: bool = False                             # a flag with `report` alone still runs the non-finite test

    @property
    def active(self):
        return self.given

    @property
    def text(self):
        if not self.active:
            return 'none'
        parts = [f"{k}={getattr(self, k)!r}" for k in ('clip', 'flat', 'noisy') if getattr(self, k) is not None]
        if self.neighbors is not None:
            parts.append(f"neighbors={self.neighbors}")
        if self.report:
            parts.append("report")
        return ','.join(parts)


_GRAMMAR = "clip=K, flat=F, noisy=N, neighbors=PATH.npy, report"
_ITEMS = FlagItems("--eeg_artifact", _GRAMMAR, ('clip', 'flat', 'noisy', 'neighbors', 'report'), bare=('report',))


def load_neighbors(path, C=None):
    """The ``neighbors=`` file -> (C, C) float32: square, finite, non-negative; `C`: the electrode count it must have."""
    try:
        w = np.load(path, allow_pickle=False)
    except (OSError, ValueError) as e:
        raise ValueError(f"--eeg_artifact: neighbors={path} cannot be read ({e}); expected {_GRAMMAR}") from None
    if w.ndim != 2 or w.shape[0] != w.shape[1] or w.shape[0] == 0 or not np.issubdtype(w.dtype, np.number):
        raise ValueError(f"--eeg_artifact: neighbors={path} holds {w.dtype} {w.shape}, not a square matrix; expected {_GRAMMAR}")
    w = np.ascontiguousarray(w, dtype=np.float32)
    check_weights(w)
    if C is not None and w.shape[0] != int(C):
        raise ValueError(f"--eeg_artifact: neighbors={path} is {w.shape[0]} x {w.shape[0]}, the shards have {int(C)} electrodes")
    return w


def check_weights(w):
    if not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError("--eeg_artifact: the neighbour weights hold a negative or non-finite value")


def parse_eeg_artifact(text):
    """``none`` / ``''`` / None, or a comma list of ``clip=K`` (> 0), ``flat=F`` (in [0, 1)), ``noisy=N`` (> 1),
    ``neighbors=PATH.npy`` (a square non-negative matrix; read here once to refuse a bad file early) and ``report`` (any subset, any
    order) -> EEGArtifactSpec.  Unknown or repeated keys and values outside those ranges raise ValueError."""
    if isinstance(text, EEGArtifactSpec):
        return text
    text = _ITEMS.clean(text)
    if text is None:
        return EEGArtifactSpec()
    got = {}
    for key, val in _ITEMS.items(text):
        if key == 'report':
            got[key] = True
        elif key == 'neighbors':
            got[key] = val
        else:
            got[key] = _ITEMS.number(key, val)
    if 'clip' in got and not got['clip'] > 0:
        raise ValueError(f"--eeg_artifact: clip={got['clip']:g} must be positive; expected {_GRAMMAR}")
    if 'flat' in got and not 0 <= got['flat'] < 1:
        raise ValueError(f"--eeg_artifact: flat={got['flat']:g} outside [0, 1); expected {_GRAMMAR}")
    if 'noisy' in got and not got['noisy'] > 1:
        raise ValueError(f"--eeg_artifact: noisy={got['noisy']:g} must be above 1; expected {_GRAMMAR}")
    if 'neighbors' in got:
        load_neighbors(got['neighbors'])
    return EEGArtifactSpec(given=True, **got)


# -------------------------------------------------------------------------------------------------------- the rule, in numpy
def kernel_keys(clip, flat, noisy):
    """The three keys as the kernels take them, fp32: 0 for an absent key, and ``flat=0`` as the smallest positive fp32."""
    k = np.float32(0 if clip is None else clip)
    n = np.float32(0 if noisy is None else noisy)
    f = np.float32(0) if flat is None else np.float32(flat)
    if flat is not None and not f > 0:
        f = np.nextafter(np.float32(0), np.float32(1))
    return k, f, n


def lower_median(v):
    """(..., n) -> (...): the element of rank (n - 1) // 2 along the last axis"""
    return np.sort(v, axis=-1)[..., (v.shape[-1] - 1) // 2]


def row_stats(x):
    """x (C, T) fp32 -> (stats (C, 2) fp32, finite (C,) bool): (m, s) per row, (0, 0) for a row with a non-finite sample"""
    finite = np.isfinite(x).all(axis=-1)
    stats = np.zeros((x.shape[0], 2), dtype=np.float32)
    if finite.any():
        xf = x[finite]
        m = lower_median(xf) + np.float32(0)                                   # -0.0 -> +0.0
        stats[finite, 0] = m
        stats[finite, 1] = lower_median(np.abs(xf - m[:, None]))
    return stats, finite


def verdicts(stats, finite, flat, noisy):
    """-> (C,) uint8 codes from the rows' scales; `flat` / `noisy` as kernel_keys gives them (0: the test is off)"""
    s = stats[:, 1]
    nf = int(finite.sum())
    ref = np.sort(s[finite])[(nf - 1) // 2] if nf else np.float32(0)
    code = np.zeros(len(s), dtype=np.uint8)
    if noisy > 0:
        code[s > noisy * ref] = NOISY
    if flat > 0:
        code[s <= flat * ref] = FLAT
    code[~finite] = NONFINITE
    if not (code == GOOD).any():
        code[code != GOOD] = UNREPAIRED
    return code


def _sample(x, k, f, n, w, repair64):
    stats, finite = row_stats(x)
    code = verdicts(stats, finite, f, n)
    m, s = stats[:, 0:1], stats[:, 1:2]
    y = x.copy()
    if k > 0:
        r = (k * MAD_TO_SIGMA) * s
        lo, hi = m - r, m + r
        with np.errstate(invalid='ignore'):
            y = np.where(x < lo, lo, np.where(x > hi, hi, x))
    y[~finite] = 0.0
    good = np.flatnonzero(code == GOOD)
    bad = np.flatnonzero((code >= FLAT) & (code <= NONFINITE))
    if repair64:
        y = y.astype(np.float64)
    if len(bad):
        cen = (y[good] - m[good].astype(y.dtype))                              # fp32: one rounding each; float64: exact
        for c in bad:
            wj = np.ones(len(good), dtype=np.float32) if w is None else w[c, good].astype(np.float32)
            if not wj.sum(dtype=np.float64) > 0:
                wj = np.ones(len(good), dtype=np.float32)
            if repair64:
                y[c] = (wj.astype(np.float64)[:, None] * cen).sum(axis=0) / wj.sum(dtype=np.float64)
            else:
                acc = np.zeros(x.shape[1], dtype=np.float32)
                for i in range(len(good)):
                    acc = acc + wj[i] * cen[i]
                y[c] = acc / np.float32(wj.sum(dtype=np.float64))
    return y, code, stats


def artifact_numpy(x, clip=None, flat=None, noisy=None, w=None, repair64=False):
    """The rule: x (B, C, T) or (C, T) float32 -> (y, verdict uint8, stats (.., C, 2) float32).  y is float32 and, outside the
    repaired rows, bit for bit the device's; with `repair64` y is float64 and the repaired rows are the float64 evaluation of the
    repair on the same fp32 inputs, unrounded.  `w`: (C, C) weights or None."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim not in (2, 3):
        raise ValueError(f"artifact_numpy: expected (B, C, T) or (C, T), got {x.shape}")
    k, f, n = kernel_keys(clip, flat, noisy)
    if w is not None:
        w = np.asarray(w, dtype=np.float32)
        check_weights(w)
        if w.shape != (x.shape[-2], x.shape[-2]):
            raise ValueError(f"artifact_numpy: weights of shape {w.shape} for {x.shape[-2]} electrodes")
    if x.ndim == 2:
        return _sample(x, k, f, n, w, repair64)
    parts = [_sample(xb, k, f, n, w, repair64) for xb in x]
    return tuple(np.stack([p[i] for p in parts]) for i in range(3))


# ------------------------------------------------------------------------------------------------------------- the stage
class ResolvedArtifact:
    """A spec resolved against the electrodes that reach the stage: `w` (C, C) float32 or None; `report`: the counts of
    report_pass, None until one was made."""
    name = 'artifact'                               # the stage protocol of data_provider/eeg_chain.py: name and four methods

    def __init__(self, spec, w=None):
        self.spec, self.w, self.report = spec, w, None
        self.keys = dict(clip=spec.clip, flat=spec.flat, noisy=spec.noisy)

    def apply(self, x, repair64=False):
        """the rule on host trials (B, C, T) or (C, T) -> (y, verdict, stats)"""
        return artifact_numpy(x, w=self.w, repair64=repair64, **self.keys)

    out_shape = lambda self, C, T: (C, T)
    apply_item = lambda self, x, group: self.apply(x)[0]

    def device_op(self, device):
        """x (B,C,T) on `device` -> (out, verdict, stats): stats launch + apply launches; the weights are uploaded now"""
        import torch
        from ign_hip import ops
        w = None if self.w is None else torch.from_numpy(self.w).to(device)
        return lambda x: ops.eeg_artifact(x.float(), neighbors=w, **self.keys)

    def device_fn(self, device):
        """x (B,C,T), gid -> the clamped / repaired rows (B,C,T); the group ids are not the stage's business"""
        run = self.device_op(device)
        return lambda x, gid: run(x)[0]

    def report_pass(self, batches, device=None):
        """One pass over `batches` of (X (B,C,T), y, gid) -- tensors on the GPU `device` go through the kernels, host arrays through
        the rule -> self.report: per electrode the trials judged flat / noisy / nonfinite / unrepaired, the trial count and the number
        of trials with any repaired electrode."""
        import torch
        run, total, trials, repaired = None, None, 0, 0
        for x, _, _ in batches:
            if torch.is_tensor(x) and x.is_cuda:
                run = run or self.device_op(x.device)
                v = run(x)[1]
                hist = torch.stack([(v == c).sum(0) for c in range(1, 5)]).cpu().numpy().astype(np.int64)
                rep = int(((v >= FLAT) & (v <= NONFINITE)).any(1).sum())
            else:
                v = self.apply(x.numpy() if torch.is_tensor(x) else x)[1]
                hist = np.stack([(v == c).sum(0) for c in range(1, 5)]).astype(np.int64)
                rep = int(((v >= FLAT) & (v <= NONFINITE)).any(1).sum())
            total = hist if total is None else total + hist
            trials, repaired = trials + int(v.shape[0]), repaired + rep
        self.report = dict(trials=trials, repaired_trials=repaired,
                           **{CODE_NAMES[c]: ([] if total is None else total[c - 1].tolist()) for c in range(1, 5)})
        return self.report

    def report_lines(self, worst=5):
        """the short table of a report: the `worst` electrodes by judged trials, and the share of trials with any repair"""
        r = self.report
        per = np.asarray([r[k] for k in CODE_NAMES[1:]], dtype=np.int64).reshape(4, -1)
        order = np.argsort(-per.sum(0), kind='stable')[:worst]
        lines = [f"eeg_artifact: {r['trials']} training trials, {r['repaired_trials']} "
                 f"({100.0 * r['repaired_trials'] / max(r['trials'], 1):.1f}%) with a repaired electrode",
                 "eeg_artifact: electrode  flat  noisy  nonfinite  unrepaired"]
        lines += [f"eeg_artifact: {int(c):9d} {per[0, c]:5d} {per[1, c]:6d} {per[2, c]:10d} {per[3, c]:11d}" for c in order if per[:, c].sum()]
        return lines

    def save(self, directory):
        """eeg_artifact.json: the spec, the weight matrix's shape and checksum, and the report if one was made."""
        path = os.path.join(directory, FILE_NAME)
        rec = dict(spec=self.spec.text, clip=self.spec.clip, flat=self.spec.flat, noisy=self.spec.noisy,
                   codes={n: c for c, n in enumerate(CODE_NAMES)},
                   weights=None if self.w is None else dict(shape=list(self.w.shape), sha256=hashlib.sha256(self.w.tobytes()).hexdigest()))
        if self.report is not None:
            rec['report'] = self.report
        with open(path, 'w') as f:
            json.dump(rec, f, indent=1)
        return path


def resolve_artifact(spec, C, T):
    """Spec (or text) + the shape of the raw items -> ResolvedArtifact: reads the weights, refuses what the kernels refuse."""
    spec = parse_eeg_artifact(spec)
    C, T = int(C), int(T)
    if T > MAX_ROW:
        raise ValueError(f"--eeg_artifact: rows of {T} samples exceed the {MAX_ROW} staged samples of the kernel")
    if C > MAX_CHANNELS:
        raise ValueError(f"--eeg_artifact: {C} electrodes exceed the {MAX_CHANNELS} of the kernel")
    return ResolvedArtifact(spec, None if spec.neighbors is None else load_neighbors(spec.neighbors, C))
