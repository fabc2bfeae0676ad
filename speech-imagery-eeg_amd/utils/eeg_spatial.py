"""Spatial filter stage (``--eeg_spatial``): the flag's parser, the composition of the re-reference and the montage matrix, a numpy
restatement of the two rules that ``ign_eeg_spatial_nct`` / ``ign_eeg_gram_nct`` (``ops.eeg_spatial`` / ``ops.eeg_gram``) run, and the
fit of the Euclidean alignment (He & Wu 2020) over the training split -- what the CPU item path applies per item and what the tests
compare the kernels against.  The stage acts across electrodes, on the raw batch, in front of everything else:

    y[b] = W[g(b)] . x[b]            W (G, Cs, Cin), one matrix per group of samples (per subject)

    p[c]    = x[b,c,0]                                   the pivot: the row's first sample
    xc[c,t] = x[b,c,t] - p[c]
    a[s,t]  = sum over c ascending of W[g,s,c] * xc[c,t]      (fp32: one fused multiply-add per step, from 0)
    P[s]    = the same sum of W[g,s,c] * p[c]
    y[b,s,t] = a[s,t] + P[s]

The pivot is the FIR rule's (utils/eeg_filter.py): recordings carry offsets of 1e4 uV over tens of uV of signal; with it, what varies
along t is computed at the signal's own scale and the offset enters once per row, as a constant that the standardisation removes.

    W0  = M . H        H = I - 11^T / Cin for ``ref=car`` (else I),  M the ``matrix=`` file's (Cs, Cin) or (G, Cs, Cin) (else I)
    W_g = A_g . W0_g   ``align=euclid``: A_g = R_g^(-1/2), R_g the mean spatial covariance of group g's training trials behind W0

The Gram rule (the covariance's numerator), on the stage's own output:

    xc = x - x[..., :1];  m[c] = (sum_t xc[c,t]) / T;  z = xc - m
    gram[g,i,j] = sum over b with gid[b] == g of sum_t z[b,i,t] * z[b,j,t];   count[g] = number of such b

No scipy in this module; torch only where ``fit_alignment`` and the stage's ``device_fn`` meet device tensors.
"""
import math
import os
from typing import NamedTuple, Optional

import numpy as np

from utils.flag_items import FlagItems

MAX_CHANNELS, MAX_GROUPS = 512, 64                  # IGN_EEG_SPATIAL_MAX_CHANNELS, IGN_EEG_SPATIAL_MAX_GROUPS
FILE_NAME = "eeg_spatial.npz"


class EEGSpatialSpec(NamedTuple):
    """The parsed ``--eeg_spatial`` flag."""
    ref: str = 'none'                               # 'none' | 'car'
    matrix: Optional[str] = None                    # path of a (Cs, Cin) or (G, Cs, Cin) .npy
    align: str = 'none'                             # 'none' | 'euclid'
    rtol: float = 1e-6                              # eigenvalues <= rtol * the largest are not inverted

    @property
    def active(self):
        return self.ref != 'none' or self.matrix is not None or self.align != 'none'

    @property
    def text(self):
        if not self.active:
            return 'none'
        parts = ([f"ref={self.ref}"] if self.ref != 'none' else []) + ([f"matrix={self.matrix}"] if self.matrix else [])
        if self.align != 'none':
            parts += [f"align={self.align}", f"rtol={self.rtol:g}"]
        return ','.join(parts)


_ITEMS = FlagItems("--eeg_spatial", "ref=car, matrix=PATH.npy, align=euclid, rtol=R", ('ref', 'matrix', 'align', 'rtol'),
                   need_value=False, expected=False)


def parse_eeg_spatial(text):
    """``none`` / ``''`` / None, or a comma list of ``ref=car``, ``matrix=PATH.npy``, ``align=euclid`` and ``rtol=R`` (any subset, any
    order) -> EEGSpatialSpec.  Unknown or repeated keys, a reference other than car, an alignment other than euclid, rtol outside
    (0, 1) and a matrix file that does not exist raise ValueError."""
    if isinstance(text, EEGSpatialSpec):
        return text
    text = _ITEMS.clean(text)
    if text is None:
        return EEGSpatialSpec()
    got = {}
    for key, val in _ITEMS.items(text):
        if key == 'ref':
            if val != 'car':
                raise ValueError(f"--eeg_spatial: ref={val!r} is not car")
        elif key == 'align':
            if val != 'euclid':
                raise ValueError(f"--eeg_spatial: align={val!r} is not euclid")
        elif key == 'matrix':
            if not val or not os.path.isfile(val):
                raise ValueError(f"--eeg_spatial: matrix={val!r}: no such file")
        else:
            val = _ITEMS.number(key, val, finite=False)
            if not (math.isfinite(val) and 0.0 < val < 1.0):
                raise ValueError(f"--eeg_spatial: rtol={val} outside (0, 1)")
        got[key] = val
    return EEGSpatialSpec(**got)


def load_matrix(spec):
    """The ``matrix=`` file of a spec as float64, None without one."""
    spec = parse_eeg_spatial(spec)
    if spec.matrix is None:
        return None
    return np.asarray(np.load(spec.matrix, allow_pickle=False), dtype=np.float64)


def compose(spec, Cin, matrix=None):
    """W0 = M . H in float64, (G0, Cs, Cin): H = I - 11^T / Cin for ``ref=car`` else I; M = `matrix` (Cs, Cin) or (G, Cs, Cin) --
    None: the spec's ``matrix=`` file, and without one I.  G0 is 1 unless the matrix is 3-D."""
    spec = parse_eeg_spatial(spec)
    Cin = int(Cin)
    if not 1 <= Cin <= MAX_CHANNELS:
        raise ValueError(f"--eeg_spatial: {Cin} input channels outside 1..{MAX_CHANNELS}")
    H = np.eye(Cin) - (np.full((Cin, Cin), 1.0 / Cin) if spec.ref == 'car' else 0.0)
    M = load_matrix(spec) if matrix is None else np.asarray(matrix, dtype=np.float64)
    if M is None:
        return H[None]
    if M.ndim not in (2, 3) or M.shape[-1] != Cin or 0 in M.shape:
        raise ValueError(f"--eeg_spatial: matrix of shape {M.shape}; expected (Cs, {Cin}) or (G, Cs, {Cin})")
    if not np.isfinite(M).all():
        raise ValueError("--eeg_spatial: the matrix holds a value that is not finite")
    M = M[None] if M.ndim == 2 else M
    if M.shape[1] > MAX_CHANNELS or M.shape[0] > MAX_GROUPS:
        raise ValueError(f"--eeg_spatial: matrix of shape {M.shape} beyond {MAX_GROUPS} groups x {MAX_CHANNELS} channels")
    return M @ H


def needs_groups(spec, matrix=None):
    """Whether the stage needs per-sample group ids: an alignment, or one matrix per group (`matrix`: the loaded ``matrix=`` file)."""
    return parse_eeg_spatial(spec).align != 'none' or (matrix is not None and np.ndim(matrix) == 3)


# -------------------------------------------------------------------------------------------------------- the rules, in numpy
def spatial_numpy(x, W, gid=None, dtype=np.float64):
    """The apply rule on host arrays: x (B, Cin, T) or one item (Cin, T), W (G, Cs, Cin) or (Cs, Cin), gid (B,) ints or None (group
    0) -> (B, Cs, T) / (Cs, T) in `dtype`.  float64 is the oracle; float32 restates the kernel's arithmetic: the subtraction, every
    step of the chain (a product of two fp32 values is exact in float64; the sum is rounded to fp32 once, as fmaf does) and the final
    addition each round to fp32.  A gid outside [0, G) gives zeros for that sample."""
    x, W = np.asarray(x), np.asarray(W)
    single = x.ndim == 2
    if single:
        x = x[None]
    if x.ndim != 3 or W.ndim not in (2, 3) or W.shape[-1] != x.shape[1]:
        raise ValueError(f"spatial_numpy: x of shape {x.shape} with W of shape {W.shape}")
    W3 = W[None] if W.ndim == 2 else W
    B, Cin, T = x.shape
    G, Cs, _ = W3.shape
    g = np.zeros(B, dtype=np.int64) if gid is None else np.asarray(gid, dtype=np.int64).reshape(B)
    ok = (g >= 0) & (g < G)
    f32 = np.dtype(dtype) == np.float32
    rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if f32 else (lambda a: a)
    Wb = (W3.astype(np.float32) if f32 else W3).astype(np.float64)[np.where(ok, g, 0)]            # (B, Cs, Cin)
    xf = (x.astype(np.float32) if f32 else x).astype(np.float64)
    p = xf[:, :, :1]
    xc = rnd(xf - p)
    a = np.zeros((B, Cs, T))
    P = np.zeros((B, Cs, 1))
    for c in range(Cin):
        w = Wb[:, :, c, None]
        a = rnd(a + w * xc[:, None, c, :])
        P = rnd(P + w * p[:, None, c, :])
    y = rnd(a + P)
    y[~ok] = 0.0
    y = y.astype(dtype)
    return y[0] if single else y


def gram_numpy(x, gid=None, groups=1):
    """The Gram rule in float64: x (B, C, T), gid (B,) or None -> (gram (G, C, C) float64, count (G,) int64)."""
    x = np.asarray(x, dtype=np.float64)
    B, C, T = x.shape
    G = int(groups)
    g = np.zeros(B, dtype=np.int64) if gid is None else np.asarray(gid, dtype=np.int64).reshape(B)
    xc = x - x[:, :, :1]
    z = xc - xc.sum(axis=-1, keepdims=True) / T
    gram, count = np.zeros((G, C, C)), np.zeros(G, dtype=np.int64)
    for b in range(B):
        if 0 <= g[b] < G:
            gram[g[b]] += z[b] @ z[b].T
            count[g[b]] += 1
    return gram, count


# ------------------------------------------------------------------------------------------------------------------ the fit
def inverse_root(R, rtol):
    """The symmetric pseudo-inverse square root of a symmetric positive semi-definite matrix in float64: V diag(l^-1/2 where
    l > rtol * max l, else 0) V^T."""
    lam, V = np.linalg.eigh(0.5 * (R + R.T))
    top = float(lam.max()) if lam.size else 0.0
    keep = lam > rtol * top if top > 0.0 else np.zeros_like(lam, dtype=bool)
    inv = np.where(keep, 1.0 / np.sqrt(np.where(keep, lam, 1.0)), 0.0)
    A = (V * inv) @ V.T
    return 0.5 * (A + A.T)                            # symmetric bit for bit


def _batch_gram(x, gid, W0, groups, post=None):
    """one raw batch through the stage with W0, then `post` if given, then the Gram rule -> (gram (G, C, C), count (G,)) as float64 /
    int64 numpy, and T"""
    try:
        import torch
    except ImportError:                                                                   # numpy batches need no torch
        torch = None
    if torch is not None and torch.is_tensor(x) and x.is_cuda:
        from ign_hip import ops
        w = torch.as_tensor(W0, dtype=torch.float32).to(x.device)
        if gid is not None:
            gid = gid.to(device=x.device, dtype=torch.int32)
        y = ops.eeg_spatial(x.float(), w, gid if w.shape[0] > 1 else None)
        if post is not None:
            y = post(y)
        gram, count = ops.eeg_gram(y, gid, groups)
        return gram.double().cpu().numpy(), count.cpu().numpy().astype(np.int64), int(x.shape[-1])
    if torch is not None and torch.is_tensor(x):
        x = x.numpy()
        gid = None if gid is None else gid.numpy()
    y = spatial_numpy(x, W0, gid if np.shape(W0)[0] > 1 else None)
    if post is not None:
        y = post(y)
    gram, count = gram_numpy(y, gid, groups)
    return gram, count, int(np.shape(x)[-1])


def fit_alignment(batches, W0, groups, rtol=1e-6, notice=print, return_info=False, post=None):
    """Euclidean alignment over one ordered pass: `batches` yields raw (X (B, Cin, T), y, gid (B,) or None) -- device tensors go
    through ops.eeg_spatial and ops.eeg_gram, host tensors and arrays through the two numpy forms in float64.  W0 (G0, Cs, Cin)
    float64 with G0 in (1, groups).  The Grams and counts of all batches are summed in float64; R_g = gram_g / (count_g * T);
    A_g = inverse_root(R_g, rtol); W_g = A_g . W0_g, rounded to fp32 once -> W (groups, Cs, Cin) float32.  A group without a training
    trial takes the pooled matrix (from the sum of all groups' Grams), with one notice.  Deterministic: the same batches give the same
    bits on every rank.  return_info: also a dict with the float64 W, R (G, Cs, Cs), counts and the list of empty groups.
    `post`: a shape-keeping callable applied to W0 . x before the Gram, on both branches (--eeg_iir: the covariance of what the model
    will see, not of drift and the mains line); None: nothing runs in between."""
    W0 = np.asarray(W0, dtype=np.float64)
    W0 = W0[None] if W0.ndim == 2 else W0
    G = int(groups)
    if W0.shape[0] not in (1, G):
        raise ValueError(f"fit_alignment: W0 holds {W0.shape[0]} groups, the data {G}")
    Cs = W0.shape[1]
    gram, count, T = np.zeros((G, Cs, Cs)), np.zeros(G, dtype=np.int64), None
    for batch in batches:
        x, gid = batch[0], batch[2] if len(batch) > 2 else None
        gb, cb, Tb = _batch_gram(x, gid if G > 1 else None, W0, G, post)    # the device path rounds W0 to fp32, the host path does not
        if T is not None and Tb != T:
            raise ValueError(f"fit_alignment: trials of {Tb} and of {T} samples in one pass")
        T = Tb
        gram += gb
        count += cb
    if T is None or count.sum() == 0:
        raise ValueError("fit_alignment: no training trial")
    pooled = inverse_root(gram.sum(axis=0) / (float(count.sum()) * T), rtol)
    empty = [g for g in range(G) if count[g] == 0]
    if empty and notice is not None:
        notice(f"eeg_spatial: group(s) {empty} have no training trial; they take the pooled alignment of all {int(count.sum())} trials")
    R = np.zeros_like(gram)
    W64 = np.zeros((G, Cs, W0.shape[2]))
    for g in range(G):
        if count[g] > 0:
            R[g] = gram[g] / (float(count[g]) * T)
            A = inverse_root(R[g], rtol)
        else:
            A = pooled
        W64[g] = A @ W0[g if W0.shape[0] > 1 else 0]
    W = W64.astype(np.float32)
    return (W, dict(W64=W64, R=R, count=count, empty=empty)) if return_info else W


class SpatialStage:
    """What a data set keeps of the stage: the spec, W0 (float64, (G0, Cs, Cin)), the matrices in use W (float32; W0 rounded until an
    alignment is fitted, then (groups, Cs, Cin)), the number of groups and their labels (the ids of subject.npy, sorted)."""

    def __init__(self, spec, W0, groups=1, labels=None):
        self.spec, self.W0, self.groups = spec, W0, int(groups)
        self.labels = np.arange(self.groups) if labels is None else np.asarray(labels)
        self.W = W0.astype(np.float32)
        self.fitted = False

    name = 'spatial'                                # the stage protocol of data_provider/eeg_chain.py: name and four methods
    Cs = property(lambda self: int(self.W0.shape[1]))

    def matrix_of(self, g):
        return self.W[g if self.W.shape[0] > 1 else 0]

    out_shape = lambda self, C, T: (self.Cs, T)
    apply_item = lambda self, x, group: spatial_numpy(x, self.matrix_of(group), dtype=np.float32)

    def device_fn(self, device):
        """x (B,Cin,T), gid (B,) int32 -> W[gid[b]] . x[b] (B,Cs,T), one launch; W is read and uploaded now: the fitted one, if fitted"""
        import torch
        from ign_hip import ops
        W = torch.from_numpy(self.W).to(device)
        one_group = W.shape[0] == 1
        return lambda x, gid: ops.eeg_spatial(x.float(), W, None if one_group else gid)

    def save(self, directory):
        """eeg_spatial.npz: the record of what each virtual channel is."""
        path = os.path.join(directory, FILE_NAME)
        np.savez(path, W=self.W, labels=self.labels, spec=np.asarray(self.spec.text), fitted=np.asarray(self.fitted))
        return path
