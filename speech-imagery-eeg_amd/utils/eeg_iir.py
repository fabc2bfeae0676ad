"""Zero-phase IIR stage (``--eeg_iir``): the flag's parser, the designer of its second-order sections (Butterworth high-pass and
low-pass, notches), the resolver against a row length, and the rule that ``ign_eeg_iir_nct`` (``ops.eeg_iir``) runs, stated once in
numpy float64 -- what the CPU item path applies per item and what the tests compare the kernel against.  The stage acts along time on
every (b, c) row of the raw (B, C, T) batch, behind ``--eeg_spatial`` and in front of ``--eeg_preprocess`` / the standardisation, and
keeps layout and shape.  Drift removal (a 0.5 Hz high-pass) and mains removal (a 50 Hz notch 1-2 Hz wide) ask for thousands of FIR
taps -- more than a CHISCO row has samples -- and are short recursive filters instead.

For a row x[0..T), sections k = 0..ns-1 with (b0, b1, b2, 1, a1, a2) and a pad length P < T:

    p      = x[0];  u = float64(x) - float64(p)                      the pivot the FIR and spatial kernels already take
    ue     = [-u[P], ..., -u[1],  u[0..T),  2u[T-1]-u[T-2], ..., 2u[T-1]-u[T-1-P]]      odd extension, N = T + 2P samples
    section (transposed direct form II), state (s1, s2):
             y = b0*v + s1;   s1 = (b1*v - a1*y) + s2;   s2 = b2*v - a2*y
    zi_k   = G_k * (g_k - b0,  b2 - a2*g_k),  g_k = (b0+b1+b2)/(1+a1+a2),  G_k = prod_{j<k} g_j      steady state for a unit step
    forward:  every section's state starts at zi_k * ue[0]; sections in order over the whole extended row
    backward: the same cascade over the reversed forward output, states starting at zi_k * (its first sample)
    out[t] = float32( back[P + t] + g0 * p ),   g0 = (prod_k g_k)^2      (0 for a high-pass, 1 for a low-pass or a notch)

This is ``scipy.signal.sosfiltfilt(sos, x, padtype='odd', padlen=P)``; the pivot is an exact identity in real arithmetic (the
cascade maps a constant c to its DC gain times c in both directions) and keeps the recording's offset, 1e4 uV over tens of uV of
signal, out of the recurrence.  All arithmetic of the recurrence is float64, on the device too: the poles of a 0.5 Hz high-pass at
500 Hz sit at radius 0.996, which multiplies every rounding by ~250, and the same rule in float32 is 4.7e-5 of the row's scale away
from float64 -- outside the project's 1e-4 budget before the model has run.  In float64 the order of evaluation stops mattering
(the kernel's 64-chunk evaluation and this sequential one differ by ~1e-11 of the scale).

No scipy in this module, and torch only where the stage's ``device_fn`` meets the device.
"""
import json
import math
import os
from typing import NamedTuple, Optional

import numpy as np

from utils.flag_items import FlagItems

MAX_SECTIONS = 8                                    # IGN_EEG_IIR_MAX_SECTIONS
MAX_ROW = 8192                                      # IGN_EEG_IIR_MAX_ROW: T + 2 P samples staged as float64 in LDS
MAX_ORDER = 8
FILE_NAME = "eeg_iir.json"


class EEGIIRSpec(NamedTuple):
    """The parsed ``--eeg_iir`` flag."""
    hp: Optional[float] = None                      # Butterworth high-pass edge, Hz
    lp: Optional[float] = None                      # Butterworth low-pass edge, Hz
    order: int = 4                                  # of hp and of lp each
    notch: tuple = ()                               # notch centres, Hz, in the order given
    q: float = 30.0                                 # quality factor of every notch: bandwidth = f / q
    sfreq: float = 500.0
    pad: Optional[int] = None                       # None: 3 * (2 ns + 1 - n1), scipy's default for these designs

    @property
    def active(self):
        return self.hp is not None or self.lp is not None or bool(self.notch)

    @property
    def text(self):
        if not self.active:
            return 'none'
        parts = [f"{k}={getattr(self, k):g}" for k in ('hp', 'lp') if getattr(self, k) is not None]
        if self.hp is not None or self.lp is not None:
            parts.append(f"order={self.order}")
        if self.notch:
            parts += ["notch=" + '+'.join(f"{f:g}" for f in self.notch), f"q={self.q:g}"]
        parts.append(f"sfreq={self.sfreq:g}")
        if self.pad is not None:
            parts.append(f"pad={self.pad}")
        return ','.join(parts)


_GRAMMAR = "hp=F, lp=F, order=N, notch=F[+F...], q=Q, sfreq=F, pad=P"
_ITEMS = FlagItems("--eeg_iir", _GRAMMAR, ('hp', 'lp', 'order', 'notch', 'q', 'sfreq', 'pad'))


def parse_eeg_iir(text):
    """``none`` / ``''`` / None, or a comma list of ``hp=F``, ``lp=F``, ``order=N`` (1..8), ``notch=F[+F...]``, ``q=Q``, ``sfreq=F``
    and ``pad=P`` (any subset, any order) -> EEGIIRSpec.  Unknown or repeated keys, edges outside (0, sfreq / 2), hp >= lp, a spec
    without a filter, and more than MAX_SECTIONS sections in total raise ValueError."""
    if isinstance(text, EEGIIRSpec):
        return text
    text = _ITEMS.clean(text)
    if text is None:
        return EEGIIRSpec()
    got = {}
    for key, val in _ITEMS.items(text):
        if key in ('order', 'pad'):
            got[key] = _ITEMS.integer(key, val)
        elif key == 'notch':
            got[key] = tuple(_ITEMS.number(key, v.strip()) for v in val.split('+'))
        else:
            got[key] = _ITEMS.number(key, val)
    spec = EEGIIRSpec(**got)
    if spec.sfreq <= 0:
        raise ValueError(f"--eeg_iir: sfreq must be positive, got {spec.sfreq}; expected {_GRAMMAR}")
    if not spec.active:
        raise ValueError(f"--eeg_iir: {text!r} names no filter (hp=, lp= or notch=); expected {_GRAMMAR}")
    if not 1 <= spec.order <= MAX_ORDER:
        raise ValueError(f"--eeg_iir: order={spec.order} outside 1..{MAX_ORDER}; expected {_GRAMMAR}")
    if not spec.q > 0:
        raise ValueError(f"--eeg_iir: q={spec.q} must be positive; expected {_GRAMMAR}")
    if spec.pad is not None and spec.pad < 0:
        raise ValueError(f"--eeg_iir: pad={spec.pad} is negative; expected {_GRAMMAR}")
    nyq = spec.sfreq / 2
    for key, edges in (('hp', (spec.hp,)), ('lp', (spec.lp,)), ('notch', spec.notch)):
        for f in edges:
            if f is not None and not 0 < f < nyq:
                raise ValueError(f"--eeg_iir: {key}={f:g} Hz outside (0, {nyq:g}) Hz; expected {_GRAMMAR}")
    if spec.hp is not None and spec.lp is not None and spec.hp >= spec.lp:
        raise ValueError(f"--eeg_iir: hp={spec.hp:g} Hz is not below lp={spec.lp:g} Hz; expected {_GRAMMAR}")
    ns = section_count(spec)
    if ns > MAX_SECTIONS:
        raise ValueError(f"--eeg_iir: {spec.text} makes {ns} second-order sections, more than {MAX_SECTIONS}; expected {_GRAMMAR}")
    return spec


def section_count(spec):
    per = (spec.order + 1) // 2
    return per * ((spec.hp is not None) + (spec.lp is not None)) + len(spec.notch)


# ------------------------------------------------------------------------------------------------------------------ the design
def butter_sos(order, fc, sfreq, kind):
    """Butterworth sections (ns, 6) float64, rows (b0, b1, b2, 1, a1, a2): prototype poles exp(i pi (2k + N + 1) / (2N)), scaled by
    the pre-warped wc = 2 fs tan(pi fc / fs) (wc / pole for kind='high'), the bilinear transform, zeros at -1 (low) or +1 (high), one
    section per conjugate pair in ascending |Im| behind the first-order section of an odd order (b2 = a2 = 0), every section scaled
    to unit gain at DC (low) or at the Nyquist rate (high)."""
    N, fs = int(order), float(sfreq)
    if kind not in ('low', 'high'):
        raise ValueError(f"butter_sos: kind {kind!r} is not low or high")
    if not 1 <= N <= MAX_ORDER or not 0 < fc < fs / 2:
        raise ValueError(f"butter_sos: order {N} outside 1..{MAX_ORDER} or edge {fc} Hz outside (0, {fs / 2}) Hz")
    wc = 2.0 * fs * math.tan(math.pi * float(fc) / fs)
    proto = [complex(math.cos(a), math.sin(a)) for a in (math.pi * (2 * k + N + 1) / (2 * N) for k in range(N))]
    if N % 2:
        proto[N // 2] = complex(-1.0, 0.0)                                    # the real pole, exactly
    poles = [(2.0 * fs + s) / (2.0 * fs - s) for s in ((wc * q if kind == 'low' else wc / q) for q in proto)]
    z = -1.0 if kind == 'low' else 1.0                                        # the zeros; unit gain is taken at -z
    rows = []
    for pz in sorted((q for q in poles if abs(q.imag) <= 1e-14 * abs(q)), key=lambda q: q.real):
        a1 = -pz.real
        k = (1.0 - z * a1) / 2.0                                              # |1 - z * (-z)| = 2
        rows.append([k, -z * k, 0.0, 1.0, a1, 0.0])
    for pz in sorted((q for q in poles if q.imag > 1e-14 * abs(q)), key=lambda q: q.imag):
        a1, a2 = -2.0 * pz.real, pz.real * pz.real + pz.imag * pz.imag
        k = (1.0 - z * a1 + a2) / 4.0                                         # denominator at -z over (1 + 1)^2
        rows.append([k, -2.0 * z * k, k, 1.0, a1, a2])
    return np.asarray(rows, dtype=np.float64)


def notch_sos(f0, q, sfreq):
    """One notch section (1, 6) float64, the closed form of ``scipy.signal.iirnotch(f0, q, fs)``: w0 = 2 pi f0 / fs,
    g = 1 / (1 + tan(w0 / (2 q))), b = g [1, -2 cos w0, 1], a = [1, -2 g cos w0, 2 g - 1]."""
    w0 = 2.0 * math.pi * float(f0) / float(sfreq)
    g = 1.0 / (1.0 + math.tan(w0 / (2.0 * float(q))))
    c = math.cos(w0)
    return np.asarray([[g, -2.0 * g * c, g, 1.0, -2.0 * g * c, 2.0 * g - 1.0]], dtype=np.float64)


def design_sos(spec):
    """The cascade of a spec, (ns, 6) float64: hp sections, lp sections, then the notches as given."""
    spec = parse_eeg_iir(spec)
    parts = []
    if spec.hp is not None:
        parts.append(butter_sos(spec.order, spec.hp, spec.sfreq, 'high'))
    if spec.lp is not None:
        parts.append(butter_sos(spec.order, spec.lp, spec.sfreq, 'low'))
    parts += [notch_sos(f, spec.q, spec.sfreq) for f in spec.notch]
    if not parts:
        raise ValueError("design_sos: the spec names no filter")
    return np.concatenate(parts, axis=0)


def default_pad(sos):
    """3 * (2 ns + 1 - n1), n1 the number of first-order sections (b2 = a2 = 0): scipy's ``sosfiltfilt`` default."""
    sos = np.asarray(sos, dtype=np.float64)
    n1 = int(np.sum((sos[:, 2] == 0.0) & (sos[:, 5] == 0.0)))
    return 3 * (2 * sos.shape[0] + 1 - n1)


def check_sos(sos):
    """(ns, 6) float64 with a0 = 1, 1 <= ns <= MAX_SECTIONS, finite, every pole strictly inside the unit circle (the Jury
    conditions of 1 + a1 z^-1 + a2 z^-2: |a2| < 1 and |a1| < 1 + a2) -> the array; ValueError otherwise."""
    sos = np.asarray(sos, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6 or not 1 <= sos.shape[0] <= MAX_SECTIONS:
        raise ValueError(f"check_sos: sections of shape {sos.shape}; expected (1..{MAX_SECTIONS}, 6)")
    if not np.isfinite(sos).all():
        raise ValueError("check_sos: a coefficient is not finite")
    for k, (_, _, _, a0, a1, a2) in enumerate(sos):
        if a0 != 1.0:
            raise ValueError(f"check_sos: section {k} has a0 = {a0}, not 1")
        if not (abs(a2) < 1.0 and abs(a1) < 1.0 + a2):
            raise ValueError(f"check_sos: section {k} (a1 = {a1}, a2 = {a2}) has a pole on or outside the unit circle")
    return sos


def freq_response(sos, w):
    """H(e^{iw}) of a cascade on an array of angular frequencies (rad / sample), complex128."""
    z1 = np.exp(-1j * np.asarray(w, dtype=np.float64))
    h = np.ones_like(z1)
    for b0, b1, b2, a0, a1, a2 in np.asarray(sos, dtype=np.float64):
        h = h * (b0 + b1 * z1 + b2 * z1 * z1) / (a0 + a1 * z1 + a2 * z1 * z1)
    return h


def section_table(sos):
    """The device table (ns, 8) float64, rows (b0, b1, b2, a1, a2, zi1, zi2, 0), and g0 = (prod_k g_k)^2."""
    sos = check_sos(sos)
    table, G = np.zeros((sos.shape[0], 8)), 1.0
    for k, (b0, b1, b2, _, a1, a2) in enumerate(sos):
        g = (b0 + b1 + b2) / (1.0 + a1 + a2)
        table[k] = (b0, b1, b2, a1, a2, G * (g - b0), G * (b2 - a2 * g), 0.0)
        G *= g
    return table, float(G * G)


class ResolvedIIR(NamedTuple):
    """A spec resolved against the rows that reach the stage."""
    spec: EEGIIRSpec
    sos: np.ndarray                                 # (ns, 6) float64
    table: np.ndarray                               # (ns, 8) float64: what the kernel reads
    pad: int
    g0: float

    name = 'iir'                                    # the stage protocol of data_provider/eeg_chain.py: name and four methods
    ns = property(lambda self: int(self.sos.shape[0]))

    def apply(self, x):
        """the rule on host rows (..., T) -> float32"""
        return iir_numpy(x, self.table, self.pad, self.g0).astype(np.float32)

    out_shape = lambda self, C, T: (C, T)
    apply_item = lambda self, x, group: self.apply(x)

    def device_fn(self, device):
        """x (B,C,T), gid -> the rows filtered forward and backward (B,C,T), one launch; the float64 section table is uploaded now"""
        import torch
        from ign_hip import ops
        coef = torch.from_numpy(self.table).to(device)
        return lambda x, gid: ops.eeg_iir(x.float(), coef, pad=self.pad, g0=self.g0)

    def save(self, directory):
        """eeg_iir.json: the resolved spec and the section table."""
        path = os.path.join(directory, FILE_NAME)
        with open(path, 'w') as f:
            json.dump(dict(spec=self.spec.text, sfreq=self.spec.sfreq, pad=self.pad, g0=self.g0, sos=self.sos.tolist(),
                           table=self.table.tolist()), f, indent=1)
        return path


def resolve_iir(spec, T, sos=None):
    """Spec (or text) + the row length T -> ResolvedIIR: designs the sections (or takes `sos`), checks them, picks the pad.  Refuses
    P >= T and rows of more than MAX_ROW = T + 2 P samples."""
    spec = parse_eeg_iir(spec)
    sos = check_sos(design_sos(spec) if sos is None else sos)
    pad = default_pad(sos) if spec.pad is None else int(spec.pad)
    T = int(T)
    if pad < 0 or pad >= T:
        raise ValueError(f"--eeg_iir: pad={pad} needs rows of more than {pad} samples, got {T}")
    if T + 2 * pad > MAX_ROW:
        raise ValueError(f"--eeg_iir: rows of {T} samples with pad={pad} exceed the {MAX_ROW} staged samples of the kernel")
    table, g0 = section_table(sos)
    return ResolvedIIR(spec, sos, table, pad, g0)


# -------------------------------------------------------------------------------------------------------- the rule, in numpy
def odd_extension(u, P):
    """(..., T) -> (..., T + 2P): [-u[P] .. -u[1], u, 2u[T-1]-u[T-2] .. 2u[T-1]-u[T-1-P]]  (u[0] = 0 after the pivot)"""
    if P == 0:
        return u
    T = u.shape[-1]
    return np.concatenate([-u[..., P:0:-1], u, 2.0 * u[..., T - 1:T] - u[..., T - 2:T - 2 - P:-1] if T - 2 - P >= 0
                           else 2.0 * u[..., T - 1:T] - u[..., T - 2::-1]], axis=-1)


def _cascade(v, table, first):
    """every section in order over the rows v (R, N) in place; states start at zi_k * first (R,)"""
    for b0, b1, b2, a1, a2, z1, z2, _ in table:
        s1, s2 = z1 * first, z2 * first
        for n in range(v.shape[1]):
            w = v[:, n]
            y = b0 * w + s1
            s1 = (b1 * w - a1 * y) + s2
            s2 = b2 * w - a2 * y
            v[:, n] = y
    return v


def iir_numpy(x, table, pad, g0):
    """The rule in float64: x (..., T) -> (..., T) float64 (the caller rounds to float32 once).  `table` (ns, 8) and g0 from
    section_table()."""
    x = np.asarray(x)
    table = np.asarray(table, dtype=np.float64)
    P, T = int(pad), x.shape[-1]
    if not 0 <= P < T:
        raise ValueError(f"iir_numpy: pad={P} needs rows of more than {P} samples, got {T}")
    xf = x.astype(np.float64).reshape(-1, T)
    p = xf[:, :1]
    v = np.ascontiguousarray(odd_extension(xf - p, P))
    _cascade(v, table, v[:, 0].copy())
    v = np.ascontiguousarray(v[:, ::-1])
    _cascade(v, table, v[:, 0].copy())
    back = v[:, ::-1]
    return (back[:, P:P + T] + g0 * p).reshape(x.shape)
