"""On-device training augmentation (``--augment``): the flag's parser, the per-step seed, and a numpy restatement of the rule
that ``csrc/ign_augment.h`` defines and ``ign_augment_btc`` (``ops.augment``) runs -- what the tests compare the kernel against.

    out[b,t,c] = keepC[b,c] * keepT[b,t] * (a[b,c] * x[b, (t - s_b) mod n_b, c] + sigma * n[b,t,c])    t <  n_b
    out[b,t,c] = x[b,t,c]                                                                           t >= n_b

Every draw is Philox4x32-10 under the 64-bit per-call seed; the last counter word tags the kind of draw (sample / channel / noise)
and every transform reads a word of its own, so turning one on does not move another's draws.  No torch in this module.
"""
import math
from typing import NamedTuple

import numpy as np

from utils.flag_items import FlagItems

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK32, _SH32 = np.uint64(0xFFFFFFFF), np.uint64(32)
TAG_SAMPLE, TAG_CHANNEL, TAG_NOISE = 0, 1, 2          # IGN_AUG_TAG_*
MASK64 = (1 << 64) - 1
NOISE_MAX = math.sqrt(48.0 * math.log(2.0))           # |n| <= sqrt(-2 ln 2^-24): the smallest u1 the 24-bit uniform takes


class AugmentSpec(NamedTuple):
    """The parsed ``--augment`` flag; the field names are the keyword arguments of ``ops.augment``."""
    shift: float = 0.0
    scale: float = 0.0
    noise: float = 0.0
    channel_drop: float = 0.0
    time_mask: float = 0.0

    @property
    def active(self):
        return any(v != 0.0 for v in self)


_KEYS = {'shift': 'shift', 'scale': 'scale', 'noise': 'noise', 'chan_drop': 'channel_drop', 'time_mask': 'time_mask'}
_ITEMS = FlagItems("--augment", f"{'|'.join(_KEYS)}=VALUE", _KEYS, need_value=False, expected=False, strip_value=False)


def channel_threshold(p):
    """thr = round(p * 65536) in fp32, rounding half to even: ign_dropout_threshold / ops.dropout_threshold."""
    return int(np.rint(np.float32(p) * np.float32(65536.0)))


def parse_augment(spec):
    """``none`` / ``''`` / None, or ``shift=0.1,scale=0.1,noise=0.05,chan_drop=0.1,time_mask=0.1`` (any subset, any order) ->
    AugmentSpec.  shift, scale, chan_drop and time_mask are rates in [0, 1); noise is a standard deviation >= 0.  Unknown or
    repeated keys and values out of range raise ValueError."""
    if isinstance(spec, AugmentSpec):
        return spec
    text = _ITEMS.clean(spec)
    if text is None:
        return AugmentSpec()
    got = {}
    for key, val in _ITEMS.items(text):
        v = _ITEMS.number(key, val, finite=False)
        if key == 'noise':
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"--augment: noise must be finite and >= 0, got {v}")
        elif not 0.0 <= float(np.float32(v)) < 1.0:
            raise ValueError(f"--augment: {key} must be in [0, 1), got {v}")
        if key == 'chan_drop' and channel_threshold(v) >= 65536:
            raise ValueError(f"--augment: chan_drop={v} rounds to a keep rate of 0")
        got[key] = v
    return AugmentSpec(**{_KEYS[k]: v for k, v in got.items()})


def _splitmix64(z):
    """The output function of splitmix64 (Steele, Lea, Flood 2014) after one increment: a bijection of 64-bit integers."""
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def step_seed(base, rank, step):
    """The 64-bit seed of one augmentation call: splitmix64(splitmix64(base) + (rank << 40 | step)) mod 2^64, rank taken mod 2^24
    and step mod 2^40.  Both rounds are bijections and the sum is injective in (rank, step), so no two (rank, step) pairs of a run
    share a seed; plain Python integers, no generator is consumed."""
    word = ((int(rank) & 0xFFFFFF) << 40) | (int(step) & 0xFFFFFFFFFF)
    return _splitmix64((_splitmix64(int(base) & MASK64) + word) & MASK64)


# --------------------------------------------------------------------------------------------------------- the rule, in numpy
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays of counters (broadcast together) under one key -> four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _SH32) ^ c1 ^ k0, p1 & _MASK32, (p0 >> _SH32) ^ c3 ^ k1, p0 & _MASK32
        k0, k1 = (k0 + _W0) & _MASK32, (k1 + _W1) & _MASK32
    return c0, c1, c2, c3


def _key(seed):
    seed = int(seed) & MASK64
    return seed & 0xFFFFFFFF, seed >> 32


def sample_draws(seed, b, lengths, shift, time_mask):
    """Per-sample draws of samples `b` with lengths `lengths` -> int64 arrays (s, m0, m1): the shift s_b in [-S, S] and the masked
    span [m0, m1).  A sample of length 0 draws nothing (all zeros)."""
    b, n = np.asarray(b, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    x0, x1, x2, _ = (w.astype(np.int64) for w in philox4x32_10(b, 0, 0, TAG_SAMPLE, *_key(seed)))
    nf = n.astype(np.float32)
    S = np.minimum(np.floor(np.float32(shift) * nf).astype(np.int64), n - 1)      # the fp32 product of the kernel
    M = np.minimum(np.floor(np.float32(time_mask) * nf).astype(np.int64), n)
    live = n >= 1
    S, M = np.where(live, S, 0), np.where(live, M, 0)
    s = x0 % (2 * S + 1) - S
    m = x1 % (M + 1)
    m0 = x2 % (np.where(live, n, 0) - m + 1)
    return np.where(live, s, 0), np.where(live, m0, 0), np.where(live, m0 + m, 0)


def channel_draws(seed, b, C, scale, chan_thr, dtype=np.float32):
    """Per-(sample, channel) draws -> (a, keep) of shape (len(b), C).  dtype float32: the kernel's roundings; float64: exact."""
    b = np.asarray(b, dtype=np.int64)
    x0, x1, _, _ = philox4x32_10(b[:, None], np.arange(C)[None, :], 0, TAG_CHANNEL, *_key(seed))
    u = (x0 >> np.uint64(8)).astype(dtype) * dtype(2.0 ** -24)
    a = dtype(1.0) + dtype(np.float32(scale)) * (dtype(2.0) * u - dtype(1.0))
    return a, (x1 & np.uint64(0xFFFF)).astype(np.int64) >= int(chan_thr)


def noise_draws(seed, b, count, dtype=np.float32):
    """The standard normals of flat indices 0 .. count - 1 of samples `b` -> (len(b), count).  One call per quad of four indices;
    float32 follows the kernel's operation order (numpy's log / sin / cos, so equal to a few ulp, not bitwise), float64 is exact."""
    b = np.asarray(b, dtype=np.int64)
    nq = (count + 3) // 4
    w = philox4x32_10(np.arange(nq)[None, :], 0, b[:, None], TAG_NOISE, *_key(seed))
    out = np.empty((len(b), nq, 4), dtype=dtype)
    two_pi = dtype(np.float32(2.0 * math.pi)) if dtype == np.float32 else dtype(2.0 * math.pi)
    for pair in (0, 1):
        u1 = ((w[2 * pair] >> np.uint64(8)) + np.uint64(1)).astype(dtype) * dtype(2.0 ** -24)
        u2 = (w[2 * pair + 1] >> np.uint64(8)).astype(dtype) * dtype(2.0 ** -24)
        r = np.sqrt(dtype(-2.0) * np.log(u1))
        th = two_pi * u2
        out[:, :, 2 * pair] = r * np.cos(th)
        out[:, :, 2 * pair + 1] = r * np.sin(th)
    return out.reshape(len(b), nq * 4)[:, :count]


def augment_reference(x, seed, lengths=None, *, shift=0.0, scale=0.0, noise=0.0, channel_drop=0.0, time_mask=0.0,
                      dtype=np.float32, first_sample=0):
    """The rule applied to a host (B, T, C) array -> array of `dtype`.  float32: the kernel's arithmetic, bitwise equal to it when
    noise == 0.  float64: the same decisions (they are integer / fp32 by definition), exact values -- the reference of the noise
    tests.  `first_sample`: the batch index of row 0 (to restate a slice of a larger batch)."""
    x = np.asarray(x)
    B, T, C = x.shape
    n = np.full(B, T, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, T)
    b = np.arange(B, dtype=np.int64) + first_sample
    s, m0, m1 = sample_draws(seed, b, n, shift, time_mask)
    a, keep_c = channel_draws(seed, b, C, scale, channel_threshold(channel_drop), dtype)
    t = np.arange(T, dtype=np.int64)[None, :]
    data = t < n[:, None]                                                              # (B, T)
    src = np.where(data, (t - s[:, None]) % np.maximum(n, 1)[:, None], t)
    xs = np.take_along_axis(x, src[:, :, None], axis=1).astype(dtype)
    v = a[:, None, :] * xs
    if noise != 0.0:
        z = dtype(np.float32(noise)) * noise_draws(seed, b, T * C, dtype).reshape(B, T, C)
        v = v + z
    keep = keep_c[:, None, :] & ~((t >= m0[:, None]) & (t < m1[:, None]))[:, :, None]
    v = np.where(keep, v, dtype(0.0))
    return np.where(data[:, :, None], v, x.astype(dtype)).astype(dtype)
