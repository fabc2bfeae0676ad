"""--warp on the host (no GPU): the flag's parser, the numpy restatement of the rule (utils/warp.py restates csrc/ign_warp.h) against
the library's host entry point ign_warp_map bit for bit and against a brute-force restatement written here, the properties of the
map (monotone, fixed end points, gains in range, identity when off, draws independent of the other transforms, prob respected), the
ABI entry points and their refusals, and the wiring into the two training loops against recording stand-in ops.  The GPU side is
tests/test_gpu_warp.py; the cases are tests/warp_cases.py.

The brute force evaluates every operation in float64 and rounds it to float32 at once: for one +, -, * or / of float32 operands
that is the correctly rounded float32 result (53 >= 2 * 24 + 2 bits), so it equals the float32 rule bit for bit while sharing none
of its array code.  The statistical bound is a six-sigma condition on a correct generator at ONE fixed seed, not a measurement.

Gain bound: g = m_i + f * (m_{i+1} - m_i) with f in [0, 1] lies between two control values in exact arithmetic; its three fp32
roundings (difference, product, sum; each at most half an ulp of a value below 2) move it by less than 2^-22, the slack allowed."""
import ctypes
import math
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from warp_cases import ALL, CASES, IDS, SEED, SEED_LOW, make_input, nonfinite_input, same_bits

import speech_imagery_eeg_amd  # noqa: F401
from utils import warp as W
from utils.augment import philox4x32_10, step_seed

BTC, MAP = "ign_warp_btc", "ign_warp_map"
E_ARG, E_TOOBIG = -1001, -1003


# ---------------------------------------------------------------- parser and flag
def test_parse_accepts():
    assert W.parse_warp("none") == W.WarpSpec() and not W.parse_warp("none").active
    assert W.parse_warp("") == W.WarpSpec() and W.parse_warp(None) == W.WarpSpec() and W.parse_warp(" NONE ") == W.WarpSpec()
    assert W.WarpSpec() == (0.0, 0.0, 0.0, 4, 1.0)
    s = W.parse_warp("twarp=0.2,mwarp=0.1,wwarp=0.15,knots=6,prob=0.5")
    assert s == W.WarpSpec(twarp=0.2, mwarp=0.1, wwarp=0.15, knots=6, prob=0.5) and s.active and W.parse_warp(s) is s
    assert W.parse_warp(" wwarp=0.25 , twarp=0.5") == W.WarpSpec(twarp=0.5, wwarp=0.25)
    assert W.parse_warp("mwarp=0.3") == W.WarpSpec(mwarp=0.3) and W.parse_warp("wwarp=0.3,knots=1").knots == 1
    assert isinstance(W.parse_warp("twarp=0.1,knots=8").knots, int)
    assert not W.parse_warp("twarp=0").active
    assert set(W.WarpSpec._fields) == {"twarp", "mwarp", "wwarp", "knots", "prob"}


@pytest.mark.parametrize("bad", ["shift=0.1", "twarp", "twarp=", "twarp=abc", "twarp=1.0", "twarp=-0.1", "mwarp=1", "wwarp=1.5",
                                 "twarp=0.99999999", "twarp=nan", "twarp=inf", "twarp=0.1,twarp=0.2", "twarp=0.1;mwarp=0.1",
                                 "twarp=0.1,knots=0", "twarp=0.1,knots=9", "twarp=0.1,knots=2.5", "twarp=0.1,knots=",
                                 "twarp=0.1,prob=0", "twarp=0.1,prob=1.5", "twarp=0.1,prob=-0.1", "twarp=0.1,prob=nan",
                                 "knots=4", "prob=0.5", "knots=4,prob=0.5", "balanced"])
def test_parse_rejects(bad):
    with pytest.raises(ValueError, match="--warp"):
        W.parse_warp(bad)


def test_flag():
    import run
    p = run.build_parser()
    act = {a.option_strings[0]: a for a in p._actions if a.option_strings}["--warp"]
    assert act.default == "none" and all(k in act.help for k in ("twarp", "mwarp", "wwarp", "knots", "prob"))
    assert p.parse_args([]).warp == "none"
    assert "--warp" in run.__doc__
    a = run.get_args(["--data", "SYNTH", "--warp", "twarp=0.2,wwarp=0.1"])
    assert W.parse_warp(a.warp) == W.WarpSpec(twarp=0.2, wwarp=0.1)
    run.get_args(["--data", "SYNTH", "--task_name", "regression", "--warp", "twarp=0.2,mwarp=0.1"])
    for bad in ("twarp=2", "knots=4", "shift=0.1"):
        with pytest.raises(ValueError):
            run.get_args(["--data", "SYNTH", "--warp", bad])
    with pytest.raises(ValueError):                                   # --augment keeps refusing the key (the flag is its own)
        run.get_args(["--data", "SYNTH", "--augment", "twarp=0.1"])


# ---------------------------------------------------------------- the map: numpy against the library's host entry point
def _lib_or_skip():
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    return _lib


def _host_map(_lib, seed, b, n, spec, want_gain=True):
    phi = np.full(max(n, 1), -5.0, dtype=np.float32)
    gain = np.full(max(n, 1), -5.0, dtype=np.float32)
    rc = _lib.lib().ign_warp_map(seed, b, n, spec.twarp, spec.mwarp, spec.wwarp, spec.knots, spec.prob,
                                 phi.ctypes.data_as(_lib.c_f), gain.ctypes.data_as(_lib.c_f) if want_gain else None)
    assert rc == 0, _lib.lib().ign_last_error()
    return phi[:n], gain[:n]


def _lengths(case):
    return [case.T] * case.B if case.lens is None else list(case.lens)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_library_map_equals_the_numpy_map_bit_for_bit(case):
    _lib = _lib_or_skip()
    spec = W.WarpSpec(**case.kw)
    for b, n in enumerate(_lengths(case)):
        phi, gain = W.warp_map(case.seed, b, n, spec)
        got_phi, got_gain = _host_map(_lib, case.seed, b, n, spec)
        assert phi.dtype == gain.dtype == np.float32 and phi.shape == gain.shape == (n,)
        assert np.array_equal(phi.view(np.uint32), got_phi.view(np.uint32)), (b, n)
        assert np.array_equal(gain.view(np.uint32), got_gain.view(np.uint32)), (b, n)
    # gain_n is optional
    n = _lengths(case)[-1]
    assert np.array_equal(_host_map(_lib, case.seed, 0, n, spec, want_gain=False)[0], W.warp_map(case.seed, 0, n, spec)[0])


# ---------------------------------------------------------------- properties of the numpy rule
SPECS = [W.WarpSpec(twarp=0.3), W.WarpSpec(wwarp=0.2), W.WarpSpec(**ALL), W.WarpSpec(twarp=0.99, mwarp=0.99, wwarp=0.5, knots=8),
         W.WarpSpec(twarp=0.99, wwarp=0.999, knots=1), W.WarpSpec(twarp=0.99, wwarp=0.001, knots=8), W.WarpSpec(mwarp=0.5, knots=2)]
LENGTHS = (2, 3, 4, 5, 63, 64, 65, 100, 1000, 1651, 2048)


@pytest.mark.parametrize("spec", SPECS, ids=[str(i) for i in range(len(SPECS))])
def test_map_is_monotone_with_fixed_ends_and_gains_in_range(spec):
    windows = set()
    for n in LENGTHS:
        for b in range(24):
            phi, gain = W.warp_map(SEED, b, n, spec)
            assert phi[0] == 0 and phi[-1] == n - 1, (n, b)
            assert (np.diff(phi) >= 0).all(), (n, b)
            assert gain.min() >= 1 - spec.mwarp - 2.0 ** -22 and gain.max() <= 1 + spec.mwarp + 2.0 ** -22, (n, b)
            assert gain.min() > 0
            if spec.mwarp == 0:
                assert (gain == 1).all()
            if (spec.twarp > 0 or spec.wwarp > 0) and n >= 64:
                assert not np.array_equal(phi, np.arange(n, dtype=np.float32)), (n, b)    # the case exercises something
            _, a, Lw, c = W.sample_draws(SEED, b, n, spec.wwarp, spec.prob)
            if spec.wwarp > 0 and n >= 3:
                assert 2 <= Lw <= n - 1 and 0 <= a <= n - Lw and float(c) in (0.5, 2.0)
                windows.add(float(c))
            else:
                assert Lw == 0
    assert windows == ({0.5, 2.0} if spec.wwarp > 0 else set())                          # both window factors occur


def test_window_length_is_clamped_at_both_ends():
    for n in (3, 4, 65, 1000):
        assert W.sample_draws(SEED, 0, n, 0.001, 1.0)[2] == 2
        assert W.sample_draws(SEED, 0, n, 0.999, 1.0)[2] == n - 1
    assert W.sample_draws(SEED, 0, 100, 0.25, 1.0)[2] == 25 and W.sample_draws(SEED, 0, 2, 0.5, 1.0)[2] == 0


def test_identity_when_off_and_for_short_samples():
    x = np.random.default_rng(0).standard_normal((3, 17, 5)).astype(np.float32)
    assert np.array_equal(W.warp_reference(x, SEED), x)
    for n in (0, 1):
        phi, gain = W.warp_map(SEED, 0, n, W.WarpSpec(**ALL))
        assert np.array_equal(phi, np.arange(n, dtype=np.float32)) and (gain == 1).all()
    phi, gain = W.warp_map(SEED, 3, 40, W.WarpSpec(knots=7, prob=0.3))
    assert np.array_equal(phi, np.arange(40, dtype=np.float32)) and (gain == 1).all()
    lens = np.array([0, 1, 17])
    out = W.warp_reference(x, SEED, lens, **ALL)
    assert np.array_equal(out[:2], x[:2]) and not np.array_equal(out[2], x[2])
    # a constant sample stays constant under the time maps, and a linear ramp stays on the ramp's line
    const = np.full((1, 50, 2), 3.25, dtype=np.float32)
    assert np.array_equal(W.warp_reference(const, SEED, twarp=0.5, wwarp=0.3), const)


def test_draws_do_not_depend_on_which_transforms_are_on():
    n, b = 200, 5
    phi_t, _ = W.warp_map(SEED, b, n, W.WarpSpec(twarp=0.3))
    phi_tm, gain_tm = W.warp_map(SEED, b, n, W.WarpSpec(twarp=0.3, mwarp=0.2))
    _, gain_m = W.warp_map(SEED, b, n, W.WarpSpec(mwarp=0.2))
    _, gain_all = W.warp_map(SEED, b, n, W.WarpSpec(**ALL))
    assert np.array_equal(phi_t, phi_tm) and np.array_equal(gain_m, gain_tm) and np.array_equal(gain_m, gain_all)
    assert np.array_equal(W.knot_draws(SEED, b, 4, 1, 0.3), W.knot_draws(SEED, b, 8, 1, 0.3)[:6])      # nor on the knot count
    w0 = W.sample_draws(SEED, b, n, 0.2, 1.0)
    w1 = W.sample_draws(SEED, b, n, 0.2, 0.25)
    assert w0[1:] == w1[1:]                                            # the window does not move with prob
    # the slice of a batch is the batch's slice; another seed, another map
    x = np.random.default_rng(1).standard_normal((5, 33, 3)).astype(np.float32)
    full = W.warp_reference(x, SEED, [33, 1, 2, 17, 30], **ALL)
    assert np.array_equal(W.warp_reference(x[:2], SEED, [33, 1], **ALL), full[:2])
    assert np.array_equal(W.warp_reference(x[3:], SEED, [17, 30], first_sample=3, **ALL), full[3:])
    assert not np.array_equal(W.warp_reference(x, SEED ^ 1, [33, 1, 2, 17, 30], **ALL), full)
    assert not np.array_equal(W.warp_reference(x, SEED_LOW, **ALL), W.warp_reference(x, SEED_LOW | (1 << 40), **ALL))     # high word


def test_prob_is_respected():
    N, p = 4096, 0.25
    on = W.sample_draws(SEED, np.arange(N), np.full(N, 50), 0.2, p)[0]
    assert abs(int(on.sum()) - N * p) <= 6 * math.sqrt(N * p * (1 - p))
    assert W.sample_draws(SEED, np.arange(N), np.full(N, 50), 0.2, 1.0)[0].all()
    x = np.random.default_rng(2).standard_normal((64, 20, 2)).astype(np.float32)
    out = W.warp_reference(x, SEED, prob=0.5, **ALL)
    same = np.array([np.array_equal(out[b], x[b]) for b in range(64)])
    assert np.array_equal(~same, W.sample_draws(SEED, np.arange(64), np.full(64, 20), 0.2, 0.5)[0]) and 10 < same.sum() < 54


# ---------------------------------------------------------------- warp_reference against a brute-force restatement
def _r(v):
    return float(np.float32(v))                       # one float32 rounding of a float64 value


def _word(seed, c0, c1, k):
    return int(philox4x32_10(c0, c1, 0, 3, seed & 0xFFFFFFFF, seed >> 32)[k])


def _brute_row(seed, b, n, twarp, mwarp, wwarp, knots, prob):
    """-> None (the sample is copied) or per output step (i0, w, g), plain loops"""
    twarp, mwarp, wwarp, prob = _r(twarp), _r(mwarp), _r(wwarp), _r(prob)
    if n < 2 or not (twarp > 0 or mwarp > 0 or wwarp > 0) or not (_word(seed, b, 0, 0) >> 8) * 2.0 ** -24 < prob:
        return None
    seg, last = knots + 1, float(n - 1)
    unit = lambda word: _r(2.0 * ((word >> 8) * 2.0 ** -24) - 1.0)
    v = [_r(1.0 + _r(twarp * unit(_word(seed, b, 1 + (i >> 2), i & 3)))) for i in range(knots + 2)]
    m = [_r(1.0 + _r(mwarp * unit(_word(seed, b, 4 + (i >> 2), i & 3)))) for i in range(knots + 2)]
    cum = [0.0]
    for i in range(seg):
        cum.append(_r(cum[i] + _r(0.5 * _r(v[i] + v[i + 1]))))
    Lw = 0
    if wwarp > 0 and n >= 3:
        Lw = min(max(int(math.floor(_r(wwarp * n))), 2), n - 1)
        a = _word(seed, b, 0, 1) % (n - Lw + 1)
        c = 2.0 if _word(seed, b, 0, 2) & 1 else 0.5

    def seg_of(p):
        u = _r(_r(p * seg) / last)
        i = min(int(math.floor(u)), knots)
        return i, _r(u - i)
    rows = []
    for t in range(n):
        p = float(t)
        if Lw:
            integral = lambda q: q + (c - 1.0) * min(max(q - a, 0.0), float(Lw))          # multiples of 0.5: exact
            p = _r(_r(integral(p) * last) / integral(last))
        if twarp > 0:
            i, f = seg_of(p)
            integ = _r(cum[i] + _r(_r(f * v[i]) + _r(_r(f * f) * _r(0.5 * _r(v[i + 1] - v[i])))))
            p = _r(_r(integ * last) / cum[seg])
        p = last if t == n - 1 else min(max(p, 0.0), last)
        i0 = min(int(math.floor(p)), n - 2)
        g = 1.0
        if mwarp > 0:
            i, f = seg_of(float(t))
            g = _r(m[i] + _r(f * _r(m[i + 1] - m[i])))
        rows.append((i0, _r(p - i0), g))
    return rows


def _brute(x, seed, lens, twarp=0.0, mwarp=0.0, wwarp=0.0, knots=4, prob=1.0):
    out = x.copy()
    B, T, C = x.shape
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            n = T if lens is None else min(max(int(lens[b]), 0), T)
            rows = _brute_row(seed, b, n, twarp, mwarp, wwarp, knots, prob)
            for t, (i0, w, g) in enumerate(rows or ()):
                for c in range(C):
                    x0, x1 = np.float32(x[b, i0, c]), np.float32(x[b, i0 + 1, c])
                    y = x0 if w == 0 else np.float32(x0 + np.float32(np.float32(w) * np.float32(x1 - x0)))
                    out[b, t, c] = np.float32(np.float32(g) * y) if _r(mwarp) > 0 else y
    return out


_BRUTE_IDS = [c.id for c in CASES if c.B * c.T * c.C <= 5 * 65 * 65]


@pytest.fixture(scope="module")
def references():
    """warp_reference of every case, computed once (the GPU tests compute their own)"""
    memo = {}

    def get(case):
        if case.id not in memo:
            x, lens = make_input(case)
            memo[case.id] = (x, lens, W.warp_reference(x, case.seed, lens, **case.kw))
            memo[case.id][2].setflags(write=False)
        return memo[case.id]
    return get


@pytest.mark.parametrize("case", [c for c in CASES if c.id in _BRUTE_IDS], ids=_BRUTE_IDS)
def test_reference_equals_the_brute_force(references, case):
    x, lens, want = references(case)
    assert want.dtype == np.float32 and same_bits(want, _brute(x, case.seed, lens, **case.kw))
    if lens is not None:
        for b, n in enumerate(lens):
            assert np.array_equal(want[b, n:], x[b, n:])              # padding untouched
            if n < 2:
                assert np.array_equal(want[b], x[b])
    if case.T >= 63:
        assert not np.array_equal(want, x)                            # the case exercises something


def test_reference_nonfinite_rows_do_not_leak_through_weight_zero():
    x = nonfinite_input()
    for kw in (dict(twarp=0.3), dict(ALL)):
        out = W.warp_reference(x, SEED, **kw)
        assert same_bits(out, _brute(x, SEED, None, **kw))
        if "mwarp" not in kw:
            assert np.array_equal(out[:, 0].view(np.uint32), x[:, 0].view(np.uint32))      # a copy: the -inf stays, no NaN appears
        assert np.isfinite(out[0, 0]).all() and np.isfinite(out[1, 0, [0, 1, 3]]).all() and out[1, 0, 2] == -np.inf
        assert not np.isfinite(out[0, 1:3]).all()                     # the non-finite row does reach its true neighbours


# ---------------------------------------------------------------- ABI
def _header_params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
    assert m, name
    return [re.split(r"[\s*]+", p.strip())[-1] for p in m.group(1).split(",")]


def test_new_symbols_are_declared_bound_and_exported():
    from ign_hip import _lib
    assert _header_params(BTC) == ["x_btc", "out_btc", "len_b", "B", "T", "C", "seed", "twarp", "mwarp", "wwarp", "knots", "prob",
                                   "stream"]
    assert _header_params(MAP) == ["seed", "b", "n", "twarp", "mwarp", "wwarp", "knots", "prob", "phi_n", "gain_n"]
    vp, ci, cf, ull = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_ulonglong
    assert _lib.SIGNATURES[BTC] == (ci, [vp] * 3 + [ci] * 3 + [ull, cf, cf, cf, ci, cf, vp])
    assert _lib.SIGNATURES[MAP] == (ci, [ull, ci, ci, cf, cf, cf, ci, cf, _lib.c_f, _lib.c_f])
    hdr = open(os.path.join(ROOT, "include", "ign_abi.h")).read()
    assert re.search(r"#define\s+IGN_WARP_MAX_T\s+\(1 << 20\)", hdr) and W.MAX_T == 1 << 20
    assert (W.MAX_T * (W.MAX_KNOTS + 1)) < 2 ** 24                     # t * seg stays exact in fp32
    rule = open(os.path.join(ROOT, "speech-imagery-eeg_amd", "csrc", "ign_warp.h")).read()
    code = re.sub(r"//[^\n]*", "", rule)
    assert not re.search(r"\b(fmaf?|expf|logf|sinf|cosf|sincosf)\s*\(", code)            # one rounding per operation, restatable
    _lib_or_skip()
    h = ctypes.CDLL(_lib.lib_path())
    assert hasattr(h, BTC) and hasattr(h, MAP)


def test_entry_points_refuse_bad_arguments_without_a_device():
    """every refusal returns before a launch: the pointers are not device memory and no GPU is needed to run this"""
    h = _lib_or_skip().lib()
    p, q = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)

    def warp(x=p, out=q, B=2, T=8, C=3, twarp=0.2, mwarp=0.1, wwarp=0.1, knots=4, prob=1.0):
        return h.ign_warp_btc(x, out, None, B, T, C, 7, twarp, mwarp, wwarp, knots, prob, None)
    assert warp(out=p) == E_ARG and b"overlap" in h.ign_last_error()
    assert warp(out=ctypes.c_void_p((1 << 20) + 4 * (2 * 8 * 3 - 1))) == E_ARG                # the last element of x
    assert warp(x=ctypes.c_void_p((1 << 24) + 4)) == E_ARG                                    # x begins inside out
    nan = float("nan")
    for kw in (dict(twarp=1.0), dict(mwarp=1.0), dict(wwarp=1.0), dict(twarp=-0.1), dict(mwarp=nan), dict(wwarp=nan),
               dict(knots=0), dict(knots=9), dict(knots=-1), dict(prob=0.0), dict(prob=1.5), dict(prob=-0.5), dict(prob=nan),
               dict(T=0), dict(B=0), dict(C=0), dict(x=None), dict(out=None)):
        assert warp(**kw) == E_ARG, kw
        assert b"ign_warp_btc" in h.ign_last_error()
    assert warp(T=(1 << 20) + 1, C=1, out=ctypes.c_void_p(1 << 60)) == E_TOOBIG               # IGN_WARP_MAX_T
    assert warp(T=1 << 20, C=1 << 11, out=ctypes.c_void_p(1 << 60)) == E_TOOBIG               # T * C beyond a 32-bit index

    buf = (ctypes.c_float * 8)()

    def wmap(b=0, n=8, twarp=0.2, mwarp=0.1, wwarp=0.1, knots=4, prob=1.0, phi=buf):
        return h.ign_warp_map(7, b, n, twarp, mwarp, wwarp, knots, prob, phi, None)
    assert wmap() == 0
    for kw in (dict(twarp=1.0), dict(mwarp=-0.5), dict(wwarp=nan), dict(knots=0), dict(knots=9), dict(prob=0.0), dict(prob=2.0),
               dict(b=-1), dict(n=-1), dict(phi=None)):
        assert wmap(**kw) == E_ARG, kw
        assert b"ign_warp_map" in h.ign_last_error()
    assert wmap(n=(1 << 20) + 1) == E_TOOBIG
    assert wmap(n=0) == 0


# ---------------------------------------------------------------- ops.warp and the training loops, against stand-ins
class _StandIn:
    """Every attribute is an entry point that records (name, args) and answers 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_ops_warp_checks_its_input_and_passes_the_rule_through(monkeypatch):
    from ign_hip import _lib, ops
    rec = _StandIn()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "check", lambda rc, what: None)
    monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(0x5EED))
    x = torch.randn(2, 8, 3)
    with pytest.raises(_lib.IgnError):                                 # no CPU fallback
        ops.warp(x, 1, twarp=0.1)
    assert not rec.calls
    monkeypatch.setattr(ops, "_need_gpu", lambda name, *ts: None)
    monkeypatch.setattr(ops, "_lengths", lambda name, lengths, B: lengths)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)         # the query needs a device
    lens = torch.tensor([8, 5], dtype=torch.int32)
    out = ops.warp(x, SEED + 2 ** 64, lengths=lens, twarp=0.2, mwarp=0.1, wwarp=0.3, knots=6, prob=0.5)
    (call,) = rec.calls
    name, args = call
    params = _header_params(BTC)
    assert name == BTC and len(args) == len(params) == len(_lib.SIGNATURES[BTC][1])
    got = dict(zip(params, (a.value if isinstance(a, ctypes.c_void_p) else a for a in args)))
    assert got["x_btc"] == x.data_ptr() and got["out_btc"] == out.data_ptr() != x.data_ptr() and got["len_b"] == lens.data_ptr()
    assert (got["B"], got["T"], got["C"], got["seed"], got["knots"], got["stream"]) == (2, 8, 3, SEED, 6, 0x5EED)
    assert (got["twarp"], got["mwarp"], got["wwarp"], got["prob"]) == (0.2, 0.1, 0.3, 0.5)
    assert out.shape == x.shape and out.dtype == x.dtype
    ops.warp(x, 1)                                                     # every rate 0: still the one launch (a copy)
    assert len(rec.calls) == 2 and rec.calls[-1][1][2] is None
    n = len(rec.calls)
    for bad in (dict(twarp=1.0), dict(mwarp=-0.25), dict(wwarp=float("nan")), dict(twarp=0.1, knots=0), dict(twarp=0.1, knots=9),
                dict(twarp=0.1, knots=2.5), dict(twarp=0.1, prob=0.0), dict(twarp=0.1, prob=1.5)):
        with pytest.raises(ValueError):
            ops.warp(x, 1, **bad)
    with pytest.raises(_lib.IgnError):
        ops.warp(x.clone().requires_grad_(True), 1, twarp=0.1)
    with pytest.raises(_lib.IgnError):
        ops.warp(x.permute(0, 2, 1), 1, twarp=0.1)
    with pytest.raises(_lib.IgnError):
        ops.warp(x[0], 1, twarp=0.1)
    assert len(rec.calls) == n                                         # refusals record no call
    assert ops.warp(torch.empty(0, 8, 3), 1, twarp=0.1).shape == (0, 8, 3) and len(rec.calls) == n


class _Stop(Exception):
    pass


def _bare_experiment(monkeypatch, order, graphed, **flags):
    """An Experiment with nothing behind it but what the two training loops touch before the forward pass, which stops the loop;
    the ops of the three batch transforms are recording stand-ins."""
    from exp import experiment_classification as E

    def op(name):
        def fn(x, *a, **k):
            order.append((name, a, k))
            return x + 1.0
        return fn
    for name in ("warp", "augment", "mix"):
        monkeypatch.setattr(E.ign_ops, name, op(name))
    e = object.__new__(E.Experiment)
    e.args = Namespace(amp=False, gradient_accumulation_steps=1, seed=11, batch_size=999, model="SBM", train_epochs=2,
                       beta_schedule="constant", task_name="classification", **flags)
    e.rank, e.device, e.distributed = 3, torch.device("cpu"), False
    e.model = torch.nn.Identity()
    e.optimizer = Namespace(schedule=Namespace(active=True), capturable=True)
    B, T, C = 4, 12, 2
    mask = torch.ones(B, T)
    mask[1, 7:] = 0
    e.train_loader = [(torch.zeros(B, T, C), torch.arange(B) % 2, mask)] * 2
    e._to_device = lambda x, y, m: (x, y, m)
    e._graph_eligible = lambda amp: graphed

    def forward(batch_x, padding_mask):
        order.append(("forward", (float(batch_x.mean()),), {}))
        raise _Stop
    e._forward = forward
    e._resolve_train_transforms()
    return e


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "hipgraph"])
def test_training_loops_warp_then_augment_then_mix_with_the_step_seed(monkeypatch, graphed):
    order = []
    e = _bare_experiment(monkeypatch, order, graphed, warp="twarp=0.2,mwarp=0.1,knots=3,prob=0.5", augment="shift=0.1", mix="mixup=0.4")
    assert e._transforms.warp == W.WarpSpec(twarp=0.2, mwarp=0.1, knots=3, prob=0.5) and e._transforms.base == 11
    with pytest.raises(_Stop):
        e.train_one_epoch(0, 40)
    assert [o[0] for o in order] == ["warp", "augment", "mix", "forward"]
    assert order[-1][1] == (3.0,)                                      # each stand-in added 1: the forward saw all three
    _, a, k = order[0]
    assert a == (step_seed(11, 3, 41),)                                # the per-step seed: base --seed, this rank, the running step
    assert k["lengths"].dtype == torch.int32 and k["lengths"].tolist() == [12, 7, 12, 12]
    assert {n: v for n, v in k.items() if n != "lengths"} == dict(twarp=0.2, mwarp=0.1, wwarp=0.0, knots=3, prob=0.5)
    assert order[1][1] == (step_seed(11, 3, 41),)                      # --augment's seed rule
    # ranks and steps differ
    assert len({step_seed(11, r, s) for r in range(4) for s in range(40, 44)}) == 16


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "hipgraph"])
@pytest.mark.parametrize("flags", [dict(warp="none"), dict(), dict(warp=" None "), dict(warp="twarp=0")], ids=["none", "absent", "None", "zero"])
def test_no_call_when_the_flag_is_off(monkeypatch, graphed, flags):
    order = []
    e = _bare_experiment(monkeypatch, order, graphed, **flags)
    assert e._transforms.warp is None and e._transforms.base is None and not e._transforms
    x = torch.zeros(2, 3, 1)
    out, soft = e._transforms(x, None, None, 1)                        # nothing is touched: no mask sum, no seed arithmetic
    assert out is x and soft == ()
    with pytest.raises(_Stop):
        e.train_one_epoch(0, 0)
    assert [o[0] for o in order] == ["forward"] and order[0][1] == (0.0,)


def test_none_is_not_parsed_beyond_the_word(monkeypatch):
    def refuse(spec):
        raise AssertionError("--warp none must not reach the parser")
    monkeypatch.setattr(W, "parse_warp", refuse)
    e = _bare_experiment(monkeypatch, [], False, warp="none")
    assert e._transforms.warp is None
    with pytest.raises(AssertionError):
        _bare_experiment(monkeypatch, [], False, warp="twarp=0.2")
    monkeypatch.undo()
    with pytest.raises(ValueError):
        _bare_experiment(monkeypatch, [], False, warp="twarp=2")


def test_only_the_training_loops_warp():
    """the chain is called from the two training loops and nowhere else, and the three ops from the chain alone: validation, test,
    saliency, the k-means initialisation, the projection, the alignment fit and the artifact report have no call"""
    chain, ops = {}, {}
    base = os.path.join(ROOT, "speech-imagery-eeg_amd")
    for folder, _, files in os.walk(base):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(folder, f)).read()
                rel = os.path.relpath(os.path.join(folder, f), base)
                for found, pattern in ((chain, r"\._transforms\("), (ops, r"ops\.(?:warp|augment|mix)\(")):
                    n = len(re.findall(pattern, text))
                    if n:
                        found[rel] = n
    assert chain == {os.path.join("exp", "experiment_classification.py"): 2}             # the two loops
    assert ops == {os.path.join("utils", "train_transforms.py"): 3}                      # one call of each op
    import inspect
    from exp import experiment_classification as E
    from utils import train_transforms as TT
    for fn in (E.Experiment.train_one_epoch, E.Experiment._train_one_epoch_graphed):
        assert inspect.getsource(fn).count("self._transforms(") == 1
    assert TT.ORDER == ("warp", "augment", "mix")                     # the order is the chain's, as data
    for fn in (E.Experiment.validation, E.Experiment.test):
        assert "_transforms" not in inspect.getsource(fn) and "_warp" not in inspect.getsource(fn)
