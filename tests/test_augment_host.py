"""--augment on the host (no GPU): the numpy restatement's Philox against the Random123 known-answer vectors, the flag's parser, the
per-step seed, the ABI entry, and the statistics and purity of the restated rule (utils/augment.py restates csrc/ign_augment.h).
The statistical bounds are six-sigma conditions on a correct generator at ONE fixed seed, not measurements."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import speech_imagery_eeg_amd  # noqa: F401
from utils import augment as A

SEED = 0x5EED0A06C0FFEE11
B, T, C = 64, 128, 128                                   # 2^20 draws


# ---------------------------------------------------------------- generator
def test_philox_known_answers():
    """kat_vectors of Random123 (philox4x32, 10 rounds)"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = A.philox4x32_10(*ctr, *key)
        assert tuple(int(w) for w in got) == want
    # and over arrays: the three counters at once under the last key differ from the scalar calls only in shape
    c = np.array([k[0] for k in kat], dtype=np.uint64).T
    got = A.philox4x32_10(c[0], c[1], c[2], c[3], *kat[2][1])
    assert tuple(int(w[2]) for w in got) == kat[2][2]


# ---------------------------------------------------------------- parser and seed
def test_parse_accepts():
    assert A.parse_augment("none") == A.AugmentSpec() and not A.parse_augment("none").active
    assert A.parse_augment("") == A.AugmentSpec() and A.parse_augment(None) == A.AugmentSpec()
    s = A.parse_augment("shift=0.1,scale=0.2,noise=0.05,chan_drop=0.3,time_mask=0.4")
    assert s == A.AugmentSpec(shift=0.1, scale=0.2, noise=0.05, channel_drop=0.3, time_mask=0.4) and s.active
    assert A.parse_augment(" time_mask=0.25 , shift=0.5") == A.AugmentSpec(shift=0.5, time_mask=0.25)
    assert A.parse_augment("noise=2.5").noise == 2.5                 # a standard deviation, not a rate
    assert not A.parse_augment("shift=0").active
    assert A.parse_augment(s) is s


@pytest.mark.parametrize("bad", ["mixup=0.1", "shift", "shift=", "shift=abc", "shift=1.0", "shift=-0.1", "scale=1", "time_mask=1.5",
                                 "chan_drop=1.0", "chan_drop=0.9999999", "noise=-1", "noise=inf", "noise=nan", "shift=0.1,shift=0.2",
                                 "shift=0.1;scale=0.1", "balanced"])
def test_parse_rejects(bad):
    with pytest.raises(ValueError):
        A.parse_augment(bad)


def test_step_seed_is_deterministic_and_collision_free():
    grid = {(r, s): A.step_seed(1234, r, s) for r in range(16) for s in range(1024)}
    assert all(0 <= v < 2 ** 64 for v in grid.values())
    assert len(set(grid.values())) == 16 * 1024
    assert all(A.step_seed(1234, r, s) == v for (r, s), v in list(grid.items())[::97])
    assert A.step_seed(1235, 0, 1) != A.step_seed(1234, 0, 1)
    assert A.step_seed(2 ** 64 + 5, 3, 7) == A.step_seed(5, 3, 7) and A.step_seed(-1, 0, 0) == A.step_seed(2 ** 64 - 1, 0, 0)
    # the mix spreads: consecutive steps differ in about half of the 64 bits
    flips = [bin(grid[(0, s)] ^ grid[(0, s + 1)]).count("1") for s in range(1023)]
    assert 24 < sum(flips) / len(flips) < 40


def test_flag():
    import run
    p = run.build_parser()
    act = {a.option_strings[0]: a for a in p._actions if a.option_strings}["--augment"]
    assert act.default == "none" and act.help
    assert p.parse_args([]).augment == "none"
    assert "--augment" in run.__doc__
    a = run.get_args(["--data", "SYNTH", "--augment", "shift=0.1,noise=0.05"])
    assert A.parse_augment(a.augment) == A.AugmentSpec(shift=0.1, noise=0.05)
    with pytest.raises(ValueError):
        run.get_args(["--data", "SYNTH", "--augment", "shift=2"])


def test_augment_symbol_is_declared_bound_and_exported():
    from ign_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    name = "ign_augment_btc"
    assert re.search(rf"\b{name}\s*\(", hdr), name
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 13
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    assert hasattr(ctypes.CDLL(_lib.lib_path()), name)


# ---------------------------------------------------------------- statistics of the rule at one seed
def test_noise_statistics():
    n = A.noise_draws(SEED, np.arange(B), T * C, np.float64).ravel()
    N = n.size
    assert N == 2 ** 20
    assert abs(n.mean()) <= 6 / math.sqrt(N)
    assert abs(n.var() - 1) <= 6 * math.sqrt(2 / N)
    assert np.abs(n).max() <= A.NOISE_MAX == math.sqrt(48 * math.log(2))
    n32 = A.noise_draws(SEED, np.arange(B), T * C, np.float32).ravel()
    assert n32.dtype == np.float32 and np.abs(n32 - n).max() <= 1e-5         # the fp32 operation order, to libm's accuracy


def test_shift_histogram():
    S, n, N = 5, 50, 4096                                   # floor(0.1 * 50) = 5
    s, _, _ = A.sample_draws(SEED, np.arange(N), np.full(N, n), 0.1, 0.0)
    assert s.min() == -S and s.max() == S
    p = 1 / (2 * S + 1)
    sd = math.sqrt(N * p * (1 - p))
    for v in range(-S, S + 1):
        k = int((s == v).sum())
        assert k > 0 and abs(k - N * p) <= 6 * sd, (v, k)


def test_electrode_drop_rate():
    thr = A.channel_threshold(0.3)
    assert thr == 19661                                     # round(0.3f * 65536)
    _, keep = A.channel_draws(SEED, np.arange(B * 16), C, 0.0, thr)
    N, p = keep.size, thr / 65536
    assert abs((~keep).sum() - N * p) <= 6 * math.sqrt(N * p * (1 - p))
    _, keep0 = A.channel_draws(SEED, np.arange(4), C, 0.0, 0)
    assert keep0.all()


def test_amplitude_range_and_mean():
    a, _ = A.channel_draws(SEED, np.arange(B * 16), C, 0.25, 0)
    assert a.dtype == np.float32 and a.min() >= 0.75 and a.max() <= 1.25
    assert abs(a.mean() - 1) <= 6 * (0.25 / math.sqrt(3)) / math.sqrt(a.size)
    a1, _ = A.channel_draws(SEED, np.arange(4), C, 0.0, 0)
    assert (a1 == 1).all()


def test_time_mask_spans():
    N = 4096
    for n, rate in ((40, 0.25), (33, 0.5), (1, 0.9), (2, 0.5)):
        M = int(np.floor(np.float32(rate) * np.float32(n)))
        _, m0, m1 = A.sample_draws(SEED, np.arange(N), np.full(N, n), 0.0, rate)
        m = m1 - m0
        assert set(m.tolist()) == set(range(M + 1)), (n, rate)
        assert (m0 >= 0).all() and (m1 <= n).all()
    # a ragged batch: every span inside its own sample, empty samples draw nothing
    lens = np.arange(N) % 34
    s, m0, m1 = A.sample_draws(SEED, np.arange(N), lens, 0.3, 0.3)
    assert (m0 >= 0).all() and (m1 <= lens).all() and (np.abs(s) <= np.maximum(lens - 1, 0)).all()
    assert (s[lens <= 1] == 0).all() and (m1[lens <= 1] == m0[lens <= 1]).all()


# ---------------------------------------------------------------- purity
ALL = dict(shift=0.2, scale=0.3, noise=0.5, channel_drop=0.3, time_mask=0.3)


def _x(b=6, t=20, c=5):
    return np.random.default_rng(0).standard_normal((b, t, c)).astype(np.float32)


def test_sub_batch_equals_rows_of_the_full_batch():
    x, lens = _x(), np.array([20, 1, 7, 0, 20, 13])
    full = A.augment_reference(x, SEED, lens, **ALL)
    assert np.array_equal(A.augment_reference(x[:2], SEED, lens[:2], **ALL), full[:2])
    assert np.array_equal(A.augment_reference(x[3:], SEED, lens[3:], first_sample=3, **ALL), full[3:])
    assert np.array_equal(full[3], x[3]) and np.array_equal(full[2, 7:], x[2, 7:])          # padding is copied through


def test_one_transform_does_not_move_anothers_draws():
    b = np.arange(32)
    n = np.full(32, 40)
    s_alone, _, _ = A.sample_draws(SEED, b, n, 0.2, 0.0)
    s_both, m0, m1 = A.sample_draws(SEED, b, n, 0.2, 0.4)
    _, m0_alone, m1_alone = A.sample_draws(SEED, b, n, 0.0, 0.4)
    assert np.array_equal(s_alone, s_both) and np.array_equal(m0, m0_alone) and np.array_equal(m1, m1_alone)
    a_alone, _ = A.channel_draws(SEED, b, 7, 0.3, 0)
    a_both, keep = A.channel_draws(SEED, b, 7, 0.3, 20000)
    _, keep_alone = A.channel_draws(SEED, b, 7, 0.0, 20000)
    assert np.array_equal(a_alone, a_both) and np.array_equal(keep, keep_alone)
    # through the whole rule: with everything on, the kept elements outside the span are those of (shift, scale, noise) alone
    x = _x(8, 40, 7)
    part = A.augment_reference(x, SEED, shift=0.2, scale=0.3, noise=0.5)
    full = A.augment_reference(x, SEED, **ALL)
    zero = full == 0
    assert zero.any() and not zero.all() and np.array_equal(full[~zero], part[~zero])
    # and noise alone is the difference that noise makes to the others
    quiet = A.augment_reference(x, SEED, shift=0.2, scale=0.3, dtype=np.float64)
    only = A.augment_reference(np.zeros_like(x), SEED, noise=0.5, dtype=np.float64)
    assert np.abs(A.augment_reference(x, SEED, shift=0.2, scale=0.3, noise=0.5, dtype=np.float64) - quiet - only).max() < 1e-12


def test_all_rates_zero_is_the_identity_and_seeds_matter():
    x = _x()
    assert np.array_equal(A.augment_reference(x, SEED), x)
    a, b = A.augment_reference(x, SEED, **ALL), A.augment_reference(x, SEED ^ 1, **ALL)
    assert not np.array_equal(a, b) and np.array_equal(a, A.augment_reference(x, SEED, **ALL))
