"""On-device EEG preprocessing (``--eeg_preprocess``): the flag's parser, the FIR designer, the resolution of a spec against a
data set's shape, and a numpy restatement of the rule that ``ign_eeg_preprocess_nct_to_btc`` (``ops.eeg_preprocess``) runs -- what
the CPU loader path applies per item and what the tests compare the kernel against.

    x~      the row extended by R = (M - 1) / 2 samples on each side: zeros, or numpy's pad(mode='reflect')
    f[n]    = sum_k h[k] * x~[n*q + R - k]            n < Td = ceil(Tin / q)        (a centred convolution: no delay)
    out     = (f[t] - mean) / (std + eps)  over t < Tv = min(Td, Tout), unbiased std; channels cropped / zero-padded to Cout

With ``h = firwin(20 q + 1, 1 / q, window='hamming')`` and zero extension, f is ``scipy.signal.decimate(x, q, ftype='fir',
zero_phase=True)`` -- what the reference's loader runs (IGN/data_factory/eeg_processor.py:258-381).  In reflect mode with R > 0 the
rule filters ``x - x[0]``: a constant is a fixed point of reflect-extended filtering up to the factor sum(h), and the
standardisation removes it.  No scipy and no torch in this module.
"""
import math
from typing import NamedTuple, Optional

import numpy as np

MAX_TAPS, MAX_DECIMATE = 1023, 16                   # IGN_EEG_MAX_TAPS, IGN_EEG_MAX_DECIMATE
EDGES = {'reflect': 0, 'zero': 1}                   # IGN_EDGE_REFLECT, IGN_EDGE_ZERO


class EEGPreprocessSpec(NamedTuple):
    """The parsed ``--eeg_preprocess`` flag."""
    sfreq: float = 500.0
    lo: Optional[float] = None
    hi: Optional[float] = None
    decimate: int = 1
    taps: Optional[int] = None
    edge: str = 'reflect'
    fit: bool = False

    @property
    def active(self):
        return self.lo is not None or self.hi is not None or self.decimate > 1 or self.fit


class Resolved(NamedTuple):
    """A spec resolved against one data set: ``resolve`` returns it; the fields are the arguments of ``ops.eeg_preprocess``."""
    taps: np.ndarray
    q: int
    edge: str
    Cout: int
    Tout: int
    Tv: int


_KEYS = ('sfreq', 'band', 'decimate', 'taps', 'edge', 'fit')


def _number(key, val):
    try:
        v = float(val)
    except ValueError:
        raise ValueError(f"--eeg_preprocess: {key}={val!r} is not a number") from None
    if not math.isfinite(v):
        raise ValueError(f"--eeg_preprocess: {key}={val!r} is not finite")
    return v


def parse_eeg_preprocess(text):
    """``none`` / ``''`` / None, or a comma list of ``sfreq=F``, ``band=LO:HI`` (either side may be empty), ``decimate=Q``,
    ``taps=M``, ``edge=reflect|zero`` and ``fit`` (any subset, any order) -> EEGPreprocessSpec.  Unknown or repeated keys, values
    out of range and an upper edge above the decimated Nyquist rate sfreq / (2 Q) (it would alias) raise ValueError."""
    if isinstance(text, EEGPreprocessSpec):
        return text
    text = '' if text is None else str(text).strip()
    if text.lower() in ('', 'none'):
        return EEGPreprocessSpec()
    got = {}
    for item in text.split(','):
        key, eq, val = item.partition('=')
        key, val = key.strip(), val.strip()
        if key not in _KEYS or (key == 'fit') == bool(eq):
            raise ValueError(f"--eeg_preprocess: {item!r} is not one of sfreq=F, band=LO:HI, decimate=Q, taps=M, edge=reflect|zero, fit")
        if key in got:
            raise ValueError(f"--eeg_preprocess: {key} given twice")
        if key == 'fit':
            got['fit'] = True
        elif key == 'edge':
            if val not in EDGES:
                raise ValueError(f"--eeg_preprocess: edge={val!r} is neither reflect nor zero")
            got['edge'] = val
        elif key == 'band':
            lo, colon, hi = val.partition(':')
            if not colon:
                raise ValueError(f"--eeg_preprocess: band={val!r} is not LO:HI")
            got['band'] = tuple(_number('band', v) if v.strip() else None for v in (lo, hi))
        elif key == 'sfreq':
            got['sfreq'] = _number(key, val)
        else:
            v = _number(key, val)
            if v != int(v):
                raise ValueError(f"--eeg_preprocess: {key}={val!r} is not an integer")
            got[key] = int(v)
    sfreq = got.get('sfreq', 500.0)
    if sfreq <= 0:
        raise ValueError(f"--eeg_preprocess: sfreq must be positive, got {sfreq}")
    q = got.get('decimate', 1)
    if not 1 <= q <= MAX_DECIMATE:
        raise ValueError(f"--eeg_preprocess: decimate={q} outside 1..{MAX_DECIMATE}")
    lo, hi = got.get('band', (None, None))
    lo = None if lo is None or lo == 0 else lo
    nyq = sfreq / (2 * q)
    if lo is not None and not 0 < lo < sfreq / 2:
        raise ValueError(f"--eeg_preprocess: lower band edge {lo} Hz outside (0, {sfreq / 2}) Hz")
    if hi is not None:
        if hi > nyq:
            raise ValueError(f"--eeg_preprocess: upper band edge {hi} Hz is above {nyq} Hz = sfreq / (2 * decimate): it would alias")
        if not 0 < hi < sfreq / 2:
            raise ValueError(f"--eeg_preprocess: upper band edge {hi} Hz outside (0, {sfreq / 2}) Hz")
    hi_eff = hi if hi is not None else (nyq if q > 1 else None)
    if lo is not None and hi_eff is not None and lo >= hi_eff:
        raise ValueError(f"--eeg_preprocess: empty band {lo}:{hi_eff} Hz")
    m = got.get('taps')
    if m is not None:
        if not (1 <= m <= MAX_TAPS and m % 2 == 1):
            raise ValueError(f"--eeg_preprocess: taps={m} must be odd and in 1..{MAX_TAPS}")
        if lo is None and hi_eff is None:
            raise ValueError("--eeg_preprocess: taps= without band= or decimate=: there is nothing to filter")
    return EEGPreprocessSpec(sfreq=sfreq, lo=lo, hi=hi, decimate=q, taps=m, edge=got.get('edge', 'reflect'),
                             fit=got.get('fit', False))


def design_fir(sfreq, lo, hi, numtaps):
    """Hamming windowed-sinc FIR taps (float64), scaled as ``scipy.signal.firwin`` scales them: low-pass (lo None) to unit gain
    at DC, band-pass at the band centre, high-pass (hi None) at the Nyquist rate.  `numtaps` is odd."""
    numtaps = int(numtaps)
    if numtaps < 1 or numtaps % 2 == 0:
        raise ValueError(f"design_fir: numtaps={numtaps} must be odd and positive")
    left = 0.0 if lo is None else 2.0 * float(lo) / float(sfreq)            # band edges as fractions of the Nyquist rate
    right = 1.0 if hi is None else 2.0 * float(hi) / float(sfreq)
    if not 0.0 <= left < right <= 1.0 or (left == 0.0 and right == 1.0):
        raise ValueError(f"design_fir: band {lo}:{hi} Hz at sfreq {sfreq} Hz is not inside (0, sfreq / 2)")
    m = np.arange(numtaps, dtype=np.float64) - 0.5 * (numtaps - 1)
    h = right * np.sinc(right * m) - left * np.sinc(left * m)
    if numtaps > 1:
        h = h * (0.54 + 0.46 * np.cos(np.linspace(-np.pi, np.pi, numtaps)))
    centre = 0.0 if left == 0.0 else 1.0 if right == 1.0 else 0.5 * (left + right)
    return h / np.sum(h * np.cos(np.pi * m * centre))


def default_numtaps(spec, notice=print):
    """``taps=`` if given; 20 Q + 1 when only decimating (scipy.signal.decimate's choice); else the smallest odd number
    >= 3.3 * sfreq / d with d the lowest non-zero band edge (the Hamming window's transition width), capped at MAX_TAPS."""
    if spec.taps is not None:
        return spec.taps
    if spec.lo is None and spec.hi is None:
        return 20 * spec.decimate + 1 if spec.decimate > 1 else 1
    hi_eff = spec.hi if spec.hi is not None else (spec.sfreq / (2 * spec.decimate) if spec.decimate > 1 else None)
    d = min(v for v in (spec.lo, hi_eff) if v is not None)
    m = int(math.ceil(3.3 * spec.sfreq / d - 1e-9))
    m += 1 - m % 2
    if m > MAX_TAPS:
        if notice is not None:
            notice(f"eeg_preprocess: a {d:g} Hz edge at {spec.sfreq:g} Hz asks for {m} taps; capped at {MAX_TAPS} "
                   f"(the transition band is wider than 3.3 * sfreq / taps suggests)")
        m = MAX_TAPS
    return m


def spec_taps(spec, notice=print):
    """The float64 taps of a spec: ``[1.0]`` with neither a band nor decimation, else design_fir over the effective band."""
    hi_eff = spec.hi if spec.hi is not None else (spec.sfreq / (2 * spec.decimate) if spec.decimate > 1 else None)
    if spec.lo is None and hi_eff is None:
        return np.ones(1, dtype=np.float64)
    return design_fir(spec.sfreq, spec.lo, hi_eff, default_numtaps(spec, notice))


def resolve(spec, Cin, Tin, target_channels=None, target_timepoints=None, notice=print):
    """A spec against raw items of shape (Cin, Tin) -> Resolved(taps, q, edge, Cout, Tout, Tv).  With ``fit`` the output shape is
    target_channels x target_timepoints, else Cin x Td.  ValueError where the launcher would refuse: a reflect halo longer than
    the row, fewer than two valid time steps."""
    spec = parse_eeg_preprocess(spec)
    Cin, Tin, q = int(Cin), int(Tin), int(spec.decimate)
    taps = spec_taps(spec, notice)
    R = (len(taps) - 1) // 2
    if spec.edge == 'reflect' and R >= Tin:
        raise ValueError(f"--eeg_preprocess: {len(taps)} taps reflect {R} samples about each end, but the rows have {Tin}; "
                         f"give a shorter filter (taps=M) or edge=zero")
    Td = -(-Tin // q)
    if spec.fit:
        if target_channels is None or target_timepoints is None:
            raise ValueError("--eeg_preprocess: fit needs --target_channels and --target_timepoints")
        Cout, Tout = int(target_channels), int(target_timepoints)
        if Cout < 1 or Tout < 1:
            raise ValueError(f"--eeg_preprocess: fit to {Cout} channels x {Tout} time points")
    else:
        Cout, Tout = Cin, Td
    Tv = min(Td, Tout)
    if Tv < 2:
        raise ValueError(f"--eeg_preprocess: {Tv} valid time step(s) after decimating {Tin} samples by {q} and fitting to {Tout}; "
                         f"the standardisation needs at least 2")
    return Resolved(taps, q, spec.edge, Cout, Tout, Tv)


# --------------------------------------------------------------------------------------------------------- the rule, in numpy
def filter_decimate(x, taps, q=1, edge='reflect', dtype=np.float64):
    """f of the rule for rows along the last axis: (..., Tin) -> (..., Td) in `dtype`, taps accumulated in ascending k.  float64
    is the oracle; float32 is a plain restatement of the kernel's arithmetic (taps rounded to fp32, the reflect pivot taken)."""
    if edge not in EDGES:
        raise ValueError(f"edge={edge!r} is neither reflect nor zero")
    x = np.asarray(x).astype(dtype)
    h = np.asarray(taps).astype(dtype)
    M, Tin, q = len(h), x.shape[-1], int(q)
    if M % 2 == 0:
        raise ValueError(f"{M} taps: the centred filter needs an odd count")
    R = (M - 1) // 2
    pad = [(0, 0)] * (x.ndim - 1) + [(R, R)]
    if edge == 'reflect':
        if R >= Tin:
            raise ValueError(f"reflect extension by {R} samples of a row of {Tin}")
        xe = np.pad(x - x[..., :1] if R > 0 else x, pad, mode='reflect')       # a single tap extends nothing: no pivot
    else:
        xe = np.pad(x, pad, mode='constant')
    Td = -(-Tin // q)
    f = np.zeros(x.shape[:-1] + (Td,), dtype=dtype)
    for k in range(M):                                # x~[n q + R - k] is xe[n q + 2 R - k]
        s = 2 * R - k
        f += h[k] * xe[..., s:s + (Td - 1) * q + 1:q]
    return f


def preprocess_numpy(x_nct, taps, q=1, edge='reflect', channels=None, timepoints=None, eps=1e-8, dtype=np.float64,
                     standardise=True):
    """The whole rule on host arrays: (..., Cin, Tin) -> (..., Tv, Cout) in `dtype` -- the valid time steps only, time first (the
    item form the loader's collate function pads to Tout and masks).  `channels` / `timepoints`: Cout / Tout, None = Cin / Td.
    standardise=False stops after the filter, decimation and fitting."""
    x = np.asarray(x_nct)
    f = filter_decimate(x, taps, q, edge, dtype)
    Cin, Td = f.shape[-2], f.shape[-1]
    Cout = Cin if channels is None else int(channels)
    Tv = Td if timepoints is None else min(Td, int(timepoints))
    Cv = min(Cin, Cout)
    f = f[..., :Cv, :Tv]
    if standardise:
        if Tv < 2:
            raise ValueError(f"{Tv} valid time step(s): the unbiased standard deviation needs 2")
        m = f.mean(axis=-1, keepdims=True)
        s = f.std(axis=-1, ddof=1, keepdims=True)
        f = (f - m) / (s + dtype(eps))
    out = np.zeros(f.shape[:-2] + (Tv, Cout), dtype=dtype)
    out[..., :Cv] = np.swapaxes(f, -1, -2)
    return out


def pad_time(out_tvc, Tout):
    """(..., Tv, C) -> ((..., Tout, C) zero-padded, mask (Tout,) bool): the batch form of ops.eeg_preprocess."""
    Tv = out_tvc.shape[-2]
    full = np.zeros(out_tvc.shape[:-2] + (int(Tout), out_tvc.shape[-1]), dtype=out_tvc.dtype)
    full[..., :Tv, :] = out_tvc
    return full, np.arange(int(Tout)) < Tv
