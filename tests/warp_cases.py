"""The cases the --warp tests share (tests/test_warp_host.py on the host, tests/test_gpu_warp.py on the GPU): the smallest shapes at
which the rule or the kernel can still go wrong.  Not a test module.

Kernel branches (csrc/ign_warp.hip): 16-byte units for C = 4, 64, 1028; 8-byte units for C = 122; single floats for C = 1, 3, 63, 65;
a row narrower than a wave (several rows per wave) for C <= 122 and wider than the block's 256 lanes for C = 1028 (two trips); one
tile per sample and several (C = 122: 33 rows per tile, so T = 63 / 64 / 65 sit around the second tile's edge; C = 1: 256 rows per
tile with T = 300; C = 1028: 3 rows per tile with T = 5).  Rule branches (csrc/ign_warp.h): n = 0, 1, 2 (no window map), 3, T = 1;
each transform alone and all three; 1 and 8 knots; twarp = 0.99; the window length clamped to 2 (wwarp = 0.001) and to n - 1
(wwarp = 0.999); prob = 0.5; a seed with and without a high word.

Input: randn plus a per-channel offset in [-2, 2]; the padding of a ragged batch holds a sentinel, not zero."""
from collections import namedtuple

import numpy as np

SEED = 0x0123456789ABCDEF                                 # non-zero high word
SEED_LOW = 0x5EED                                         # zero high word
SENTINEL = 777.0
ALL = dict(twarp=0.3, mwarp=0.2, wwarp=0.2)

Case = namedtuple("Case", "id B T C lens seed kw")


def _c(id, B, T, C, lens=None, seed=SEED, **kw):
    return Case(id, B, T, C, lens, seed, kw or dict(ALL))


CASES = [
    _c("T1-1x1x3", 1, 1, 3),
    _c("tiny-n-5x5x3", 5, 5, 3, (0, 1, 2, 3, 5)),
    _c("5x63x1", 5, 63, 1),
    _c("1x300x1-tiles", 1, 300, 1),
    _c("5x65x3-knots1", 5, 65, 3, knots=1, **ALL),
    _c("1x64x4-knots8", 1, 64, 4, knots=8, **ALL),
    _c("1x64x63-low-seed", 1, 64, 63, seed=SEED_LOW),
    _c("5x63x64-twarp", 5, 63, 64, twarp=0.3),
    _c("5x63x64-mwarp", 5, 63, 64, mwarp=0.2),
    _c("5x63x64-wwarp", 5, 63, 64, wwarp=0.2),
    _c("1x65x65-twarp0.99", 1, 65, 65, twarp=0.99, mwarp=0.2, wwarp=0.2),
    _c("5x64x122-ragged", 5, 64, 122, (0, 1, 2, 32, 64)),
    _c("5x64x122-prob0.5", 5, 64, 122, prob=0.5, **ALL),
    _c("5x65x4-window-min", 5, 65, 4, (65, 3, 4, 33, 64), wwarp=0.001),
    _c("5x65x4-window-max", 5, 65, 4, (65, 3, 4, 33, 64), wwarp=0.999, twarp=0.3),
    _c("1x5x1028-wide", 1, 5, 1028),
    _c("1x1651x122", 1, 1651, 122),
]
IDS = [c.id for c in CASES]


def make_input(case):
    """-> (x float32 (B, T, C), lens int32 (B,) or None), deterministic per shape"""
    rng = np.random.default_rng(1000 * case.B + 10 * case.T + case.C)
    x = (rng.standard_normal((case.B, case.T, case.C)) + (4 * rng.random(case.C) - 2)).astype(np.float32)
    if case.lens is None:
        return x, None
    for b, n in enumerate(case.lens):
        x[b, n:] = SENTINEL
    return x, np.asarray(case.lens, dtype=np.int32)


def nonfinite_input():
    """A (2, 9, 4) batch with inf / NaN beside positions whose weight is 0: phi(0) = 0 always, so out[b, 0] is a copy of x[b, 0]
    whatever x[b, 1] holds.  Sample 0: row 1 is +inf; sample 1: row 1 is NaN and row 0 holds a -inf."""
    x = np.random.default_rng(7).standard_normal((2, 9, 4)).astype(np.float32)
    x[0, 1] = np.inf
    x[1, 1] = np.nan
    x[1, 0, 2] = -np.inf
    return x


def same_bits(a, b):
    """Bitwise equality of two float32 arrays, except that any NaN equals any NaN: the sign and payload of a NaN that arithmetic
    produces (inf - inf) is the processor's convention, not the rule's."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
