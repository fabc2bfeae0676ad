"""Rational resampling stage (``--eeg_resample``): the flag's parser, the designer of its Kaiser-windowed low-pass, the resolver
against a row length, and the rule that ``ign_eeg_resample_nct`` (``ops.eeg_resample``) runs, stated once in numpy float64 -- what
the CPU item path applies per item and what the tests compare the kernel against.  The stage acts along time on every (b, c) row of
the raw (B, C, Tin) batch, behind ``--eeg_iir`` and in front of ``--eeg_preprocess`` / the standardisation, keeps the layout and
changes the row length: Tout = ceil(Tin * up / down).  500 -> 256 Hz is 64/125, which ``decimate=Q`` cannot express.

With g = gcd(up, down) divided out, mr = max(up, down), hl = half * mr, M = 2 hl + 1:

    h[j] = up * k[j] * sinc((j - hl) / mr) / mr,   k = np.kaiser(M, beta),   normalised so that sum(h) / up = 1

-- ``scipy.signal.firwin(M, 1 / mr, window=('kaiser', beta)) * up``, the filter ``scipy.signal.resample_poly`` designs.  The taps are
rounded to float32 once, on the host.  For a row x[0..Tin):

    p  = x[0];  u = x - p                                   the pivot the FIR, spatial and IIR stages take
    ue = u extended by R = Lp samples on both sides         edge=reflect (numpy 'reflect') or edge=zero
    for n in [0, Tout):  c = n * down
        y[n] = p + sum_k h[c - k up + hl] * ue[k]           over the k with 0 <= c - k up + hl <= 2 hl, k descending

and in polyphase form, with khi = (c + hl) div up, r = (c + hl) mod up, Lp = ceil(M / up), tab[r][i] = h[r + i up] (0 past 2 hl):

    y[n] = p + sum_{i < Lp} tab[r][i] * ue[khi - i]         i ascending: one chain of Lp multiply-adds

With edge=zero, y - p is ``scipy.signal.resample_poly(u, up, down)``.  The pivot p re-enters with gain exactly 1, on purpose: the
per-phase DC gains sum_i tab[r][i] differ from 1 by up to 1.4e-4 at 64/125, so resampling a raw row prints a ripple of the
recording's offset (2e4 uV) of about 3 uV onto tens of uV of signal, and a zero extension of the raw row is off by thousands of uV
at both ends; pivoted, the filter sees the signal alone, a constant row yields p exactly, and the float32 evaluation stays an order
of magnitude closer to float64.

No scipy in this module, and torch only where the stage's ``device_fn`` meets the device.
"""
import json
import math
import os
from fractions import Fraction
from typing import NamedTuple

import numpy as np

from utils.flag_items import FlagItems

MAX_TABLE = 8192                                    # IGN_EEG_RESAMPLE_MAX_TABLE: up * Lp floats of phase table
MAX_LDS_BYTES = 64 * 1024                           # the extended row plus the padded table, staged in LDS
MAX_HALF = 32
EDGES = {'reflect': 0, 'zero': 1}                   # IGN_EDGE_REFLECT, IGN_EDGE_ZERO
FILE_NAME = "eeg_resample.json"


class EEGResampleSpec(NamedTuple):
    """The parsed ``--eeg_resample`` flag; up / down are in lowest terms, (1, 1) is no stage."""
    up: int = 1
    down: int = 1
    sfreq: float = 500.0                            # the rate of the rows that reach the stage
    half: int = 10                                  # taps reach half * max(up, down) samples of the up-sampled grid to each side
    beta: float = 5.0                               # of the Kaiser window
    edge: str = 'reflect'

    @property
    def active(self):
        return (self.up, self.down) != (1, 1)

    @property
    def rate(self):
        """the output rate in Hz"""
        return self.sfreq * self.up / self.down

    @property
    def text(self):
        if not self.active:
            return 'none'
        return f"ratio={self.up}/{self.down},sfreq={self.sfreq!r},half={self.half},beta={self.beta!r},edge={self.edge}"


_GRAMMAR = "rate=F or ratio=P/Q, sfreq=F, half=H, beta=B, edge=reflect|zero"
_ITEMS = FlagItems("--eeg_resample", _GRAMMAR, ('rate', 'ratio', 'sfreq', 'half', 'beta', 'edge'))


def _decimal(key, val):
    """a decimal string -> its exact Fraction"""
    try:
        out = Fraction(val)
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"--eeg_resample: {key}={val!r} is not a number; expected {_GRAMMAR}") from None
    if '/' in val:
        raise ValueError(f"--eeg_resample: {key}={val!r} is not a decimal number; expected {_GRAMMAR}")
    return out


def phase_count(up, down, half):
    """(hl, M, Lp) of a ratio in lowest terms"""
    hl = int(half) * max(int(up), int(down))
    M = 2 * hl + 1
    return hl, M, -(-M // int(up))


def parse_eeg_resample(text, notice=None):
    """``none`` / ``''`` / None, or a comma list of ``rate=F`` (the output rate in Hz) or ``ratio=P/Q``, ``sfreq=F`` (the input rate,
    default 500), ``half=H`` (1..32, default 10), ``beta=B`` (default 5.0) and ``edge=reflect|zero`` -> EEGResampleSpec.  up / down
    is the exact fraction rate / sfreq of the decimal strings, in lowest terms.  Unknown or repeated keys, both or neither of rate
    and ratio, non-positive numbers, half outside 1..32 and a phase table of more than MAX_TABLE floats raise ValueError.  A rate
    equal to sfreq is no stage: the inactive spec, with one line to `notice`."""
    if isinstance(text, EEGResampleSpec):
        return text
    text = _ITEMS.clean(text)
    if text is None:
        return EEGResampleSpec()
    got = {}
    for key, val in _ITEMS.items(text):
        if key == 'half':
            got[key] = _ITEMS.integer(key, val)
        elif key == 'edge':
            if val not in EDGES:
                raise ValueError(f"--eeg_resample: edge={val!r} is neither reflect nor zero; expected {_GRAMMAR}")
            got[key] = val
        elif key == 'ratio':
            p, slash, q = val.partition('/')
            if not slash:
                raise ValueError(f"--eeg_resample: ratio={val!r} is not P/Q; expected {_GRAMMAR}")
            got[key] = (_ITEMS.integer(key, p.strip()), _ITEMS.integer(key, q.strip()))
        else:
            got[key] = _decimal(key, val)
    if ('rate' in got) == ('ratio' in got):
        raise ValueError(f"--eeg_resample: {text!r} needs one of rate= and ratio=, not {'both' if 'rate' in got else 'neither'}; "
                         f"expected {_GRAMMAR}")
    sfreq = got.get('sfreq', Fraction(500))
    if sfreq <= 0:
        raise ValueError(f"--eeg_resample: sfreq must be positive, got {float(sfreq):g}; expected {_GRAMMAR}")
    if 'rate' in got:
        if got['rate'] <= 0:
            raise ValueError(f"--eeg_resample: rate must be positive, got {float(got['rate']):g}; expected {_GRAMMAR}")
        frac = got['rate'] / sfreq
    else:
        p, q = got['ratio']
        if p <= 0 or q <= 0:
            raise ValueError(f"--eeg_resample: ratio={p}/{q} must be positive; expected {_GRAMMAR}")
        frac = Fraction(p, q)
    half, beta = got.get('half', 10), float(got.get('beta', Fraction(5)))
    if not 1 <= half <= MAX_HALF:
        raise ValueError(f"--eeg_resample: half={half} outside 1..{MAX_HALF}; expected {_GRAMMAR}")
    if not (math.isfinite(beta) and beta > 0):
        raise ValueError(f"--eeg_resample: beta must be positive, got {beta:g}; expected {_GRAMMAR}")
    up, down = frac.numerator, frac.denominator
    if (up, down) == (1, 1):
        if notice is not None:
            notice(f"eeg_resample: {text} names the input rate {float(sfreq):g} Hz itself: no stage")
        return EEGResampleSpec()
    _, _, Lp = phase_count(up, down, half)
    if up * Lp > MAX_TABLE:
        raise ValueError(f"--eeg_resample: {text} is {up}/{down}: a phase table of {up} x {Lp} = {up * Lp} floats, more than "
                         f"{MAX_TABLE}; give a smaller half= or a simpler ratio=P/Q; expected {_GRAMMAR}")
    return EEGResampleSpec(up=up, down=down, sfreq=float(sfreq), half=half, beta=beta, edge=got.get('edge', 'reflect'))


def same_rate(a, b):
    """two rates in Hz, one of them possibly a rounded quotient"""
    return math.isclose(float(a), float(b), rel_tol=1e-9, abs_tol=0.0)


# ------------------------------------------------------------------------------------------------------------------ the design
def design_taps(up, down, half=10, beta=5.0):
    """The float64 taps (M,) of a ratio in lowest terms: the Kaiser-windowed sinc with its cut-off at the lower of the two Nyquist
    rates, scaled to DC gain `up` (gain 1 per phase on average)."""
    up, down = int(up), int(down)
    if up < 1 or down < 1 or math.gcd(up, down) != 1:
        raise ValueError(f"design_taps: {up}/{down} is not a positive ratio in lowest terms")
    mr = max(up, down)
    hl, M, _ = phase_count(up, down, half)
    m = (np.arange(M, dtype=np.float64) - hl) / mr
    h = np.kaiser(M, float(beta)) * np.sinc(m) / mr
    return up * (h / h.sum())


def phase_table(h, up):
    """taps (M,) -> tab (up, Lp) of the same dtype, tab[r][i] = h[r + i up], zero past the last tap"""
    h = np.asarray(h)
    up = int(up)
    Lp = -(-len(h) // up)
    full = np.zeros(up * Lp, dtype=h.dtype)
    full[:len(h)] = h
    return np.ascontiguousarray(full.reshape(Lp, up).T)


def out_length(Tin, up, down):
    return -(-int(Tin) * int(up) // int(down))


class ResolvedResample(NamedTuple):
    """A spec resolved against the rows that reach the stage."""
    spec: EEGResampleSpec
    taps: np.ndarray                                # (M,) float64, unrounded
    tab: np.ndarray                                 # (up, Lp) float32: what the kernel reads
    Tin: int
    Tout: int

    up = property(lambda self: self.spec.up)
    down = property(lambda self: self.spec.down)
    edge = property(lambda self: self.spec.edge)
    hl = property(lambda self: (len(self.taps) - 1) // 2)
    Lp = property(lambda self: int(self.tab.shape[1]))

    def apply(self, x):
        """the rule on host rows (..., Tin) -> (..., Tout) float32: float64 arithmetic on the float32 taps, rounded once"""
        return resample_numpy(x, self.tab, self.up, self.down, self.hl, self.edge).astype(np.float32)

    name = 'resample'                               # the stage protocol of data_provider/eeg_chain.py: name and four methods
    out_shape = lambda self, C, T: (C, self.Tout)
    apply_item = lambda self, x, group: self.apply(x)

    def device_fn(self, device):
        """x (B,C,Tin), gid -> the rows resampled (B,C,Tout), one launch; the fp32 phase table is uploaded now"""
        import torch
        from ign_hip import ops
        tab = torch.from_numpy(self.tab).to(device)
        return lambda x, gid: ops.eeg_resample(x.float(), tab, up=self.up, down=self.down, half_len=self.hl, edge=self.edge)

    def record(self):
        s = self.spec
        return dict(spec=s.text, sfreq_in=s.sfreq, sfreq_out=s.rate, up=s.up, down=s.down, half=s.half, beta=s.beta, edge=s.edge,
                    Tin=self.Tin, Tout=self.Tout, taps=len(self.taps), phase_len=self.Lp)

    def save(self, directory):
        """eeg_resample.json: the rates, the ratio, the filter's parameters and the row lengths."""
        path = os.path.join(directory, FILE_NAME)
        with open(path, 'w') as f:
            json.dump(self.record(), f, indent=1)
        return path


def lds_bytes(Tin, up, Lp):
    """what ign_eeg_resample_lds_bytes answers: the extended row and the table with its row stride padded odd, as floats"""
    return 4 * (int(Tin) + 2 * int(Lp) + int(up) * (int(Lp) | 1))


def resolve_resample(spec, Tin):
    """Spec (or text) + the row length Tin -> ResolvedResample, or None for an inactive spec.  Refuses what the launcher would: a
    reflect extension of R = Lp samples that does not fit the row, a row plus table beyond the LDS budget."""
    spec = parse_eeg_resample(spec)
    if not spec.active:
        return None
    Tin = int(Tin)
    taps = design_taps(spec.up, spec.down, spec.half, spec.beta)
    tab = phase_table(taps.astype(np.float32), spec.up)
    Lp = tab.shape[1]
    if Tin < 1 or (spec.edge == 'reflect' and Lp >= Tin):
        raise ValueError(f"--eeg_resample: {spec.up}/{spec.down} with half={spec.half} reflects {Lp} samples about each end, but the "
                         f"rows have {Tin}; give a smaller half= or edge=zero")
    if lds_bytes(Tin, spec.up, Lp) > MAX_LDS_BYTES:
        raise ValueError(f"--eeg_resample: rows of {Tin} samples with a {spec.up} x {Lp} phase table exceed the "
                         f"{MAX_LDS_BYTES // 1024} KB the kernel stages")
    return ResolvedResample(spec, taps, tab, Tin, out_length(Tin, spec.up, spec.down))


# -------------------------------------------------------------------------------------------------------- the rule, in numpy
def _extend(x, R, edge, dtype):
    """rows (Rw, Tin) -> (p (Rw, 1), ue (Rw, Tin + 2R)) in `dtype`"""
    if edge not in EDGES:
        raise ValueError(f"edge={edge!r} is neither reflect nor zero")
    Tin = x.shape[-1]
    if edge == 'reflect' and R >= Tin:
        raise ValueError(f"reflect extension by {R} samples of a row of {Tin}")
    p = x[:, :1]
    return p, np.pad(x - p, [(0, 0), (R, R)], mode='reflect' if edge == 'reflect' else 'constant')


def resample_numpy(x, tab, up, down, hl, edge='reflect', dtype=np.float64):
    """The rule in polyphase form: x (..., Tin) -> (..., Tout) in `dtype` (float64 is the oracle, the caller rounds once; float32 is
    a plain restatement of the kernel's arithmetic without its fused multiply-add).  `tab` (up, Lp) from phase_table()."""
    x = np.asarray(x)
    tab = np.asarray(tab).astype(dtype)
    up, down, hl = int(up), int(down), int(hl)
    Lp, Tin = tab.shape[1], x.shape[-1]
    if tab.shape[0] != up or Lp != -(-(2 * hl + 1) // up):
        raise ValueError(f"resample_numpy: a table of shape {tab.shape} for up={up}, hl={hl}")
    Tout = out_length(Tin, up, down)
    p, ue = _extend(x.astype(dtype).reshape(-1, Tin), Lp, edge, dtype)
    khi, r = np.divmod(np.arange(Tout, dtype=np.int64) * down + hl, up)
    acc = np.zeros((ue.shape[0], Tout), dtype=dtype)
    for i in range(Lp):                               # ue[k] sits at index k + R, R = Lp
        acc += tab[r, i] * ue[:, khi - i + Lp]
    return (acc + p).reshape(x.shape[:-1] + (Tout,))


def resample_direct(x, h, up, down, edge='reflect'):
    """The rule as first written, in float64, one output at a time over the taps h (M,): the k with a tap under them, descending.
    Slow; the tests hold the polyphase form against it."""
    x = np.asarray(x)
    h = np.asarray(h, dtype=np.float64)
    up, down, hl = int(up), int(down), (len(h) - 1) // 2
    Lp, Tin = -(-len(h) // up), x.shape[-1]
    Tout = out_length(Tin, up, down)
    p, ue = _extend(x.astype(np.float64).reshape(-1, Tin), Lp, edge, np.float64)
    y = np.zeros((ue.shape[0], Tout))
    for n in range(Tout):
        c = n * down
        acc = np.zeros(ue.shape[0])
        for k in range((c + hl) // up, -(-(c - hl) // up) - 1, -1):
            acc += h[c - k * up + hl] * ue[:, k + Lp]
        y[:, n] = acc
    return (y + p).reshape(x.shape[:-1] + (Tout,))
