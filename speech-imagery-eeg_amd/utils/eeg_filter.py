"""On-device EEG preprocessing (``--eeg_preprocess``): the flag's parser, the FIR designer, the resolution of a spec against a
data set's shape, and a numpy restatement of the rule that ``ign_eeg_preprocess_nct_to_btc`` (``ops.eeg_preprocess``) runs -- what
the CPU loader path applies per item and what the tests compare the kernel against.

    x~      the row extended by R = (M - 1) / 2 samples on each side: zeros, or numpy's pad(mode='reflect')
    f[n]    = sum_k h[k] * x~[n*q + R - k]            n < Td = ceil(Tin / q)        (a centred convolution: no delay)
    out     = (f[t] - mean) / (std + eps)  over t < Tv = min(Td, Tout), unbiased std; channels cropped / zero-padded to Cout

With ``h = firwin(20 q + 1, 1 / q, window='hamming')`` and zero extension, f is ``scipy.signal.decimate(x, q, ftype='fir',
zero_phase=True)`` -- what the reference's loader runs (IGN/data_factory/eeg_processor.py:258-381).  In reflect mode with R > 0 the
rule filters ``x - x[0]``: a constant is a fixed point of reflect-extended filtering up to the factor sum(h), and the
standardisation removes it.  No scipy in this module, and torch only where a stage's ``device_fn`` meets the device.

A filter bank (``bank=LO:HI+LO:HI+...``, optionally ``envelope``) runs nb bands with one common tap count over the same extended row
(``ign_eeg_filterbank_nct_to_btc`` / ``ops.eeg_filterbank``; here ``filterbank_numpy``):

    a_j[n]  = sum_k H[j,k] * x~[n*q + R - k]          the rule above, per band
    f_j     = a_j, or with ``envelope``  sqrt(a_j^2 + b_j^2),  b_j the same sum with the quadrature taps G[j] (the Hilbert pair of
              H[j], ``design_quadrature``); in fp32  sqrtf(fmaf(a, a, b * b))
    out     (..., Tv, nb*Cout), band-major: channel j*Cout + c is electrode c of band j, each block standardised and fitted as above

so block j of a plain bank is ``preprocess_numpy`` with H[j].  ``envelope`` needs ``edge=reflect`` (the pivot keeps the recording's
offset times sum(H[j]) out of the square root, where the standardisation could no longer remove it) and both edges of every band.
"""
import math
from typing import NamedTuple, Optional

import numpy as np

from utils.flag_items import FlagItems

MAX_TAPS, MAX_DECIMATE = 1023, 16                   # IGN_EEG_MAX_TAPS, IGN_EEG_MAX_DECIMATE
MAX_BANDS = 8                                       # IGN_EEG_MAX_BANDS
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
    bank: Optional[tuple] = None                    # ((lo, hi), ...) of a filter bank; lo / hi above are then None
    envelope: bool = False

    @property
    def active(self):
        return self.lo is not None or self.hi is not None or self.decimate > 1 or self.fit or self.bank is not None


# The stage protocol of data_provider/eeg_chain.py, once for Resolved and ResolvedBank; the chain's last stage: its rules standardise too.
def _apply_item(self, x, group):
    """one item (Cin, Tin) -> (Tv, channels) float32: the rule in fp32 on the fp32 taps"""
    quad = None if self.quad is None else self.quad.astype(np.float32)
    return filterbank_numpy(x, self.taps2d.astype(np.float32), quad, self.q, self.edge, self.Cout, self.Tout).astype(np.float32)


def _device_fn(self, device):
    """x (B,Cin,Tin), gid -> (X[B,Tout,channels] filtered, decimated, fitted, standardised, band-major, mask = t < Tv); uploads the taps"""
    import torch
    from ign_hip import ops
    taps = torch.as_tensor(self.taps2d, dtype=torch.float32).to(device)
    quad = None if self.quad is None else torch.as_tensor(self.quad, dtype=torch.float32).to(device)
    kw = dict(decimate=self.q, edge=self.edge, channels=self.Cout, timepoints=self.Tout)
    return lambda x, gid: ops.eeg_filterbank(x.float(), taps, quad, **kw)


class Resolved(NamedTuple):
    """A one-band spec resolved against one data set: ``resolve`` returns it; the fields are the arguments of
    ``ops.eeg_preprocess``.  The properties answer what a ResolvedBank answers, for the bank of one that it is."""
    taps: np.ndarray                                # (M,)
    q: int
    edge: str
    Cout: int
    Tout: int
    Tv: int

    quad = property(lambda self: None)
    channels = property(lambda self: self.Cout)
    taps2d = property(lambda self: self.taps[None], doc="the taps as a bank's (nb, M) = (1, M)")
    name, apply_item, device_fn = 'preprocess', _apply_item, _device_fn
    out_shape, save = (lambda self, C, T: (self.channels, self.Tout)), (lambda self, directory: None)     # no record file


class ResolvedBank(NamedTuple):
    """A bank or envelope spec resolved against one data set; the fields are the arguments of ``ops.eeg_filterbank``.  `Cout` is
    the number of electrodes PER BAND; the items have ``channels`` = nb * Cout channels, band-major."""
    taps: np.ndarray                                # (nb, M) in-phase
    quad: Optional[np.ndarray]                      # (nb, M) quadrature, None without envelope
    q: int
    edge: str
    Cout: int
    Tout: int
    Tv: int
    bands: tuple                                    # ((lo, hi), ...) in Hz; an open upper edge is sfreq / (2 Q) when decimating, else None

    channels = property(lambda self: len(self.bands) * self.Cout)
    taps2d = property(lambda self: self.taps)
    name, apply_item, device_fn = 'preprocess', _apply_item, _device_fn
    out_shape, save = (lambda self, C, T: (self.channels, self.Tout)), (lambda self, directory: None)     # no record file


def bank_channel(res, index):
    """Channel `index` of a bank's output -> (band index, (lo, hi) in Hz, electrode index): what shapelet (k, c) or a saliency
    column of a model trained on the bank belongs to."""
    index = int(index)
    if not 0 <= index < res.channels:
        raise IndexError(f"channel {index} of a bank with {res.channels} channels")
    j, c = divmod(index, res.Cout)
    return j, res.bands[j], c


_ITEMS = FlagItems("--eeg_preprocess", "sfreq=F, band=LO:HI, bank=LO:HI+LO:HI+..., decimate=Q, taps=M, edge=reflect|zero, fit, envelope",
                   ('sfreq', 'band', 'bank', 'decimate', 'taps', 'edge', 'fit', 'envelope'), bare=('fit', 'envelope'),
                   need_value=False, expected=False)
_number = _ITEMS.number


def parse_eeg_preprocess(text):
    """``none`` / ``''`` / None, or a comma list of ``sfreq=F``, ``band=LO:HI`` (either side may be empty), ``decimate=Q``,
    ``taps=M``, ``edge=reflect|zero`` and ``fit`` (any subset, any order) -> EEGPreprocessSpec.  Unknown or repeated keys, values
    out of range and an upper edge above the decimated Nyquist rate sfreq / (2 Q) (it would alias) raise ValueError.
    ``bank=LO:HI+LO:HI+...`` (1 to 8 entries, order kept, overlap allowed, each under ``band=``'s rules; not together with
    ``band=``) asks for a filter bank, ``envelope`` for the band-power envelope of every band (both edges of every band needed,
    not with ``edge=zero``); ``band=LO:HI,envelope`` is a bank of one band.  Without either the spec is what it always was."""
    if isinstance(text, EEGPreprocessSpec):
        return text
    text = _ITEMS.clean(text)
    if text is None:
        return EEGPreprocessSpec()
    got = {}
    for key, val in _ITEMS.items(text):
        if key in _ITEMS.bare:
            got[key] = True
        elif key == 'edge':
            if val not in EDGES:
                raise ValueError(f"--eeg_preprocess: edge={val!r} is neither reflect nor zero")
            got['edge'] = val
        elif key == 'band':
            lo, colon, hi = val.partition(':')
            if not colon:
                raise ValueError(f"--eeg_preprocess: band={val!r} is not LO:HI")
            got['band'] = tuple(_number('band', v) if v.strip() else None for v in (lo, hi))
        elif key == 'bank':
            bands = []
            for entry in val.split('+'):
                lo, colon, hi = entry.partition(':')
                if not colon:
                    raise ValueError(f"--eeg_preprocess: bank entry {entry!r} is not LO:HI")
                bands.append(tuple(_number('bank', v) if v.strip() else None for v in (lo, hi)))
            got['bank'] = bands
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
    envelope, edge = got.get('envelope', False), got.get('edge', 'reflect')
    if 'bank' in got and 'band' in got:
        raise ValueError("--eeg_preprocess: bank= and band= exclude each other")
    nyq = sfreq / (2 * q)

    def check_band(lo, hi):
        """band='s rules for one (lo, hi) -> (lo, hi, hi_eff)"""
        lo = None if lo is None or lo == 0 else lo
        if lo is not None and not 0 < lo < sfreq / 2:
            raise ValueError(f"--eeg_preprocess: lower band edge {lo} Hz outside (0, {sfreq / 2}) Hz")
        if hi is not None:
            if hi > nyq:
                raise ValueError(f"--eeg_preprocess: upper band edge {hi} Hz is above {nyq} Hz = sfreq / (2 * decimate): it would alias")
            if not 0 < hi < sfreq / 2:
                raise ValueError(f"--eeg_preprocess: upper band edge {hi} Hz outside (0, {sfreq / 2}) Hz")
        hi_eff = _upper_edge(sfreq, hi, q)
        if lo is not None and hi_eff is not None and lo >= hi_eff:
            raise ValueError(f"--eeg_preprocess: empty band {lo}:{hi_eff} Hz")
        return lo, hi, hi_eff

    bank = None
    if 'bank' in got or envelope:
        entries = got['bank'] if 'bank' in got else [got.get('band', (None, None))]
        if not 1 <= len(entries) <= MAX_BANDS:
            raise ValueError(f"--eeg_preprocess: bank= with {len(entries)} bands; 1..{MAX_BANDS} are supported")
        bank = []
        for lo, hi in entries:
            lo, hi, hi_eff = check_band(lo, hi)
            if lo is None and hi_eff is None:
                raise ValueError("--eeg_preprocess: a bank entry without either edge: there is nothing to filter")
            if envelope and (lo is None or hi is None):
                raise ValueError(f"--eeg_preprocess: envelope needs both edges of every band, got "
                                 f"{'' if lo is None else lo}:{'' if hi is None else hi} (a low-pass or high-pass has no envelope)")
            bank.append((lo, hi))
        bank = tuple(bank)
        if envelope and edge == 'zero':
            raise ValueError("--eeg_preprocess: envelope needs edge=reflect: with edge=zero the recording's offset is not pivoted "
                             "away, enters the square root and cannot be standardised out")
        lo = hi = hi_eff = None
    else:
        lo, hi, hi_eff = check_band(*got.get('band', (None, None)))
    m = got.get('taps')
    if m is not None:
        if not (1 <= m <= MAX_TAPS and m % 2 == 1):
            raise ValueError(f"--eeg_preprocess: taps={m} must be odd and in 1..{MAX_TAPS}")
        if bank is None and lo is None and hi_eff is None:
            raise ValueError("--eeg_preprocess: taps= without band= or decimate=: there is nothing to filter")
        if envelope and m == 1:
            raise ValueError("--eeg_preprocess: envelope with taps=1: a single tap has no quadrature pair")
    return EEGPreprocessSpec(sfreq=sfreq, lo=lo, hi=hi, decimate=q, taps=m, edge=edge, fit=got.get('fit', False), bank=bank,
                             envelope=envelope)


def design_fir(sfreq, lo, hi, numtaps):
    """Hamming windowed-sinc FIR taps (float64), scaled as ``scipy.signal.firwin`` scales them: low-pass (lo None) to unit gain
    at DC, band-pass at the band centre, high-pass (hi None) at the Nyquist rate.  `numtaps` is odd."""
    h, _, _, _, _, scale = _windowed_sinc(sfreq, lo, hi, numtaps)
    return h / scale


def _windowed_sinc(sfreq, lo, hi, numtaps):
    """-> (windowed unscaled taps, window, m = k - R, left, right, firwin's scale factor)"""
    numtaps = int(numtaps)
    if numtaps < 1 or numtaps % 2 == 0:
        raise ValueError(f"design_fir: numtaps={numtaps} must be odd and positive")
    left = 0.0 if lo is None else 2.0 * float(lo) / float(sfreq)            # band edges as fractions of the Nyquist rate
    right = 1.0 if hi is None else 2.0 * float(hi) / float(sfreq)
    if not 0.0 <= left < right <= 1.0 or (left == 0.0 and right == 1.0):
        raise ValueError(f"design_fir: band {lo}:{hi} Hz at sfreq {sfreq} Hz is not inside (0, sfreq / 2)")
    m = np.arange(numtaps, dtype=np.float64) - 0.5 * (numtaps - 1)
    h = right * np.sinc(right * m) - left * np.sinc(left * m)
    win = np.ones(numtaps)
    if numtaps > 1:
        win = 0.54 + 0.46 * np.cos(np.linspace(-np.pi, np.pi, numtaps))
        h = h * win
    centre = 0.0 if left == 0.0 else 1.0 if right == 1.0 else 0.5 * (left + right)
    return h, win, m, left, right, np.sum(h * np.cos(np.pi * m * centre))


def design_quadrature(sfreq, lo, hi, numtaps):
    """The Hilbert pair of ``design_fir(sfreq, lo, hi, numtaps)`` (float64): the ideal band's quadrature response
    (cos(pi left m) - cos(pi right m)) / (pi m), 0 at m = 0, under the same Hamming window and divided by the SAME scale factor as
    the in-phase taps (not by a sum of its own: the pair then has one gain, and sqrt(a^2 + b^2) of a sinusoid at the band centre
    is its amplitude).  Antisymmetric, so its sum is 0: a constant does not pass."""
    _, win, m, left, right, scale = _windowed_sinc(sfreq, lo, hi, numtaps)
    safe = np.where(m == 0.0, 1.0, m)
    g = np.where(m == 0.0, 0.0, (np.cos(np.pi * left * m) - np.cos(np.pi * right * m)) / (np.pi * safe))
    return g * win / scale


def _upper_edge(sfreq, hi, q):
    """the effective upper edge of a band: `hi`; an open one is sfreq / (2 Q) when decimating (the anti-aliasing low-pass), else None"""
    return hi if hi is not None else (sfreq / (2 * q) if q > 1 else None)


def _bank_edges(spec):
    """the (lo, effective hi) of every band of a spec; a one-band spec is a bank of one"""
    bands = spec.bank if spec.bank is not None else ((spec.lo, spec.hi),)
    return tuple((lo, _upper_edge(spec.sfreq, hi, spec.decimate)) for lo, hi in bands)


def default_numtaps(spec, notice=print):
    """``taps=`` if given; 20 Q + 1 when only decimating (scipy.signal.decimate's choice); else the smallest odd number
    >= 3.3 * sfreq / d with d the lowest non-zero edge of all bands (the Hamming window's transition width), capped at MAX_TAPS."""
    if spec.taps is not None:
        return spec.taps
    if spec.bank is None and spec.lo is None and spec.hi is None:
        return 20 * spec.decimate + 1 if spec.decimate > 1 else 1
    d = min(v for band in _bank_edges(spec) for v in band if v is not None)
    m = int(math.ceil(3.3 * spec.sfreq / d - 1e-9))
    m += 1 - m % 2
    if m > MAX_TAPS:
        if notice is not None:
            notice(f"eeg_preprocess: a {d:g} Hz edge at {spec.sfreq:g} Hz asks for {m} taps; capped at {MAX_TAPS} "
                   f"(the transition band is wider than 3.3 * sfreq / taps suggests)")
        m = MAX_TAPS
    return m


def bank_taps(spec, notice=print):
    """Any spec -> (H (nb, M) float64, G (nb, M) float64 or None, bands): design_fir / design_quadrature per band, one M.  A
    one-band spec gives its single row; one with neither a band nor decimation the identity ``[[1.0]]``."""
    bands = _bank_edges(spec)
    if bands == ((None, None),):
        return np.ones((1, 1), dtype=np.float64), None, bands
    M = default_numtaps(spec, notice)
    H = np.stack([design_fir(spec.sfreq, lo, hi, M) for lo, hi in bands])
    G = np.stack([design_quadrature(spec.sfreq, lo, hi, M) for lo, hi in bands]) if spec.envelope else None
    return H, G, bands


def spec_taps(spec, notice=print):
    """The float64 taps (M,) of a one-band spec: ``[1.0]`` with neither a band nor decimation, else design_fir over its band."""
    return bank_taps(spec, notice)[0][0]


def resolve(spec, Cin, Tin, target_channels=None, target_timepoints=None, notice=print):
    """A spec against raw items of shape (Cin, Tin) -> Resolved(taps, q, edge, Cout, Tout, Tv).  With ``fit`` the output shape is
    target_channels x target_timepoints, else Cin x Td.  ValueError where the launcher would refuse: a reflect halo longer than
    the row, fewer than two valid time steps.  A bank or envelope spec -> ResolvedBank(taps (nb, M), quad, q, edge, Cout, Tout, Tv,
    bands) instead; Cout (and with ``fit`` target_channels) counts electrodes PER BAND, the items have nb * Cout channels."""
    spec = parse_eeg_preprocess(spec)
    Cin, Tin, q = int(Cin), int(Tin), int(spec.decimate)
    taps, quad, bands = bank_taps(spec, notice)
    M = taps.shape[1]
    R = (M - 1) // 2
    if spec.edge == 'reflect' and R >= Tin:
        raise ValueError(f"--eeg_preprocess: {M} taps reflect {R} samples about each end, but the rows have {Tin}; "
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
    return (ResolvedBank(taps, quad, q, spec.edge, Cout, Tout, Tv, bands) if spec.bank is not None
            else Resolved(taps[0], q, spec.edge, Cout, Tout, Tv))


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
    return _fit_standardise(filter_decimate(np.asarray(x_nct), taps, q, edge, dtype), channels, timepoints, eps, dtype, standardise)


def _fit_standardise(f, channels, timepoints, eps, dtype, standardise):
    """filtered rows (..., Cin, Td) -> (..., Tv, Cout): the fitting and the standardisation of the rule"""
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


def envelope_of(a, b, dtype=np.float64):
    """sqrt(a^2 + b^2) of the in-phase and quadrature outputs.  float32 is the kernel's sqrtf(fmaf(a, a, b * b)): b * b rounded to
    fp32, a * a exact in float64 (24-bit factors), their sum rounded once to fp32."""
    if dtype == np.float32:
        a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
        return np.sqrt((a.astype(np.float64) * a.astype(np.float64) + (b * b).astype(np.float64)).astype(np.float32))
    return np.sqrt(a * a + b * b)


def filterbank_numpy(x_nct, taps, quad=None, q=1, edge='reflect', channels=None, timepoints=None, eps=1e-8, dtype=np.float64,
                     standardise=True):
    """The bank's rule on host arrays: (..., Cin, Tin) with taps (nb, M) and optional quadrature taps (nb, M) ->
    (..., Tv, nb * Cout) in `dtype`, band-major.  Block j without `quad` is preprocess_numpy(x, taps[j], ...) itself; with `quad`
    the envelope of the pair is standardised and fitted the same way."""
    H = np.asarray(taps)
    if H.ndim != 2 or not 1 <= H.shape[0] <= MAX_BANDS:
        raise ValueError(f"filterbank_numpy: taps of shape {H.shape}; expected (nb, M) with nb in 1..{MAX_BANDS}")
    G = None if quad is None else np.asarray(quad)
    if G is not None:
        if G.shape != H.shape:
            raise ValueError(f"filterbank_numpy: quad of shape {G.shape} beside taps of shape {H.shape}")
        if edge != 'reflect':
            raise ValueError("filterbank_numpy: the envelope needs edge='reflect' (the pivot keeps the offset out of the square root)")
        if H.shape[1] == 1:
            raise ValueError("filterbank_numpy: the envelope needs more than one tap")
    x = np.asarray(x_nct)
    blocks = []
    for j in range(H.shape[0]):
        f = filter_decimate(x, H[j], q, edge, dtype)
        if G is not None:
            f = envelope_of(f, filter_decimate(x, G[j], q, edge, dtype), dtype)
        blocks.append(_fit_standardise(f, channels, timepoints, eps, dtype, standardise))
    return np.concatenate(blocks, axis=-1)
