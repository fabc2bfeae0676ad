"""Input gradients through the shapelet expert, host side: the C entry points ign_shapelet_bwd_input(_bank) and ign_instnorm_bwd
(include/ign_abi.h) are declared, bound and exported; the instance-norm backward formula the kernel implements agrees with
float64 autograd; argument errors come back before any launch.  The GPU side is tests/test_gpu_input_grad.py."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUP, E_TOOBIG = -1001, -1002, -1003
SYMBOLS = ("ign_shapelet_bwd_input", "ign_shapelet_bwd_input_bank", "ign_instnorm_bwd")


def _lib_or_skip():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    return _lib.lib()


def test_input_grad_symbols_are_declared_bound_and_exported():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    for name in SYMBOLS:
        m = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name        # one ctypes entry per C parameter
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    h = ctypes.CDLL(_lib.lib_path())
    for name in SYMBOLS:
        assert hasattr(h, name), name


def test_header_states_the_tie_and_constant_row_conventions():
    hdr = open(os.path.join(ROOT, "include", "ign_abi.h")).read()
    doc = hdr[hdr.index("Backward of ign_shapelet_fwd w.r.t. the INPUT"):hdr.index("int ign_instnorm_bwd(")]
    assert "sign(0) convention" in doc and "sign(x - w) = -1" in doc
    assert "sigma == 0" in doc and "gx = 0" in doc


def test_instnorm_backward_formula_agrees_with_float64_autograd():
    """gx_j = [g_j - mean(g) - y_j (sum_i g_i y_i)/(T-1) (sigma+eps)/sigma] / (sigma+eps), restated in numpy"""
    import torch
    from oracle import ign_oracle as O
    rng = np.random.default_rng(0)
    eps = 1e-8
    for (B, T, C) in ((2, 37, 3), (1, 200, 5), (3, 2, 2)):
        x = rng.standard_normal((B, T, C)) * 3.0 + 50.0
        g = rng.standard_normal((B, C, T))
        xt = torch.from_numpy(x).requires_grad_(True)
        O.instance_norm(xt).backward(torch.from_numpy(g))
        xc = x.transpose(0, 2, 1)                                          # (B,C,T)
        mu = xc.mean(-1, keepdims=True)
        sigma = np.sqrt(((xc - mu) ** 2).sum(-1, keepdims=True) / (T - 1))
        y = (xc - mu) / (sigma + eps)
        gx = (g - g.mean(-1, keepdims=True) - y * (g * y).sum(-1, keepdims=True) / (T - 1) * (sigma + eps) / sigma) / (sigma + eps)
        np.testing.assert_allclose(gx.transpose(0, 2, 1), xt.grad.numpy(), rtol=1e-9, atol=1e-12)


def _p(v):
    return ctypes.c_void_p(v)


def _grp_args(**kw):
    a = dict(xn=_p(16), w=_p(32), g=_p(48), p=_p(64), dmin=_p(80), ld=12, col0=0, tstar=_p(96), zmu=_p(112), d=_p(128), gx=_p(144),
             acc=0, B=2, C=4, T=60, K=3, L=9, stride=1, eps=1.0, mode=0, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(mode=2), E_ARG, b"IGN_DIST_L1 and IGN_DIST_MSE only"),
    (dict(mode=3 | 0x10), E_ARG, b"IGN_DIST_L1 and IGN_DIST_MSE only"),
    (dict(mode=0x44), E_ARG, b"unknown mode"),
    (dict(gx=None), E_ARG, b"null pointer"),
    (dict(d=None), E_ARG, b"d_save is required"),
    (dict(mode=0x10, p=None), E_ARG, b"null pointer"),
    (dict(L=61), E_ARG, b"bad dimensions"),
    (dict(stride=0), E_ARG, b"bad dimensions"),
    (dict(ld=11), E_ARG, b"row pitch"),
    (dict(T=50000, L=10), E_TOOBIG, b"LDS staging"),
    (dict(T=50000, L=25000, stride=14), E_TOOBIG, b"LDS staging"),
])
def test_shapelet_bwd_input_argument_errors_need_no_device(kw, rc, msg):
    L = _lib_or_skip()
    assert L.ign_shapelet_bwd_input(*_grp_args(**kw)) == rc
    assert msg in L.ign_last_error()


def test_shapelet_bwd_input_row_limit_is_the_forwards():
    """beyond the forward's LDS staging limit both calls return IGN_E_TOOBIG, with the same message"""
    L = _lib_or_skip()
    for T, Lg, stride in ((41200, 300, 1), (50000, 1000, 9)):
        fwd = L.ign_shapelet_fwd(_p(16), _p(32), None, _p(48), _p(64), 12, 0, _p(80), _p(96), None, None, 2, 4, T, 3, Lg, stride, 1.0,
                                 0, None)
        msg_f = L.ign_last_error().split(b":", 1)[1]
        bwd = L.ign_shapelet_bwd_input(*_grp_args(T=T, L=Lg, stride=stride))
        assert fwd == bwd == E_TOOBIG and L.ign_last_error().split(b":", 1)[1] == msg_f


def test_shapelet_bwd_input_has_no_row_limit_of_its_own():
    """The launch plan of the input-gradient pass (ign_bwdx_plan, restated) stays far below the default 64 KB of LDS on every row
    the forward's staging rule (fwd_staging, restated) accepts -- strides up to T - 1 included -- so the forward's IGN_E_TOOBIG is
    the only row limit; rows the forward refuses are refused by the call itself, before any launch."""
    L = _lib_or_skip()
    seen, worst = set(), 0
    for T in (60, 1000, 3100, 17984, 40000, 41000):
        for Lg in sorted({3, 9, T // 10, T // 2, T - 1, T}):
            for stride in sorted({1, 2, 8, 14, 64, 511, 512, 513, 650, 651, 8000, T - 1}):
                Tw = (T - Lg) // stride + 1
                TT = min(16, (Tw + 63) // 64) if stride == 1 else 1
                npass = (Tw + 64 * TT - 1) // (64 * TT)
                xs_len = ((npass * 64 * TT - 1) * stride + (TT - 1) + Lg + 3) & ~3
                fits = xs_len * 4 + (6400 if npass > 1 else 0) <= 160 * 1024
                seen.add(fits)
                if not fits:
                    assert L.ign_shapelet_bwd_input(*_grp_args(T=T, L=Lg, stride=stride)) == E_TOOBIG, (T, Lg, stride)
                    assert b"a row needs" in L.ign_last_error()
                    continue
                M = (Lg + stride - 1) // stride
                mc = min(M, max(1, 512 // stride))
                na = ((1023 // stride + 1 + mc) + 3) & ~3
                worst = max(worst, 2 * (mc * stride + na + 8) * 4)
    assert seen == {True, False} and worst <= 17 * 1024


def _bank_args(G=2, **kw):
    vt, it = ctypes.c_void_p * 8, ctypes.c_int * 8
    tab = vt(*[16 * (i + 1) for i in range(8)])
    a = dict(xn=_p(16), G=G, w=tab, g=_p(48), p=_p(64), dmin=_p(80), ld=60, col0=it(0, 12, 24, 36, 48, 0, 0, 0), tstar=tab, zmu=tab, d=tab,
             gx=_p(144), B=2, C=4, T=60, K=it(*[3] * 8), L=it(9, 20, 9, 9, 9, 9, 9, 9), stride=it(*[1] * 8), eps=1.0, mode=1, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(G=0), E_ARG, b"outside 1..8"),
    (dict(G=9), E_ARG, b"outside 1..8"),
    (dict(d=None), E_ARG, b"null table"),
    (dict(mode=2), E_ARG, b"IGN_DIST_L1 and IGN_DIST_MSE only"),
    (dict(L=(ctypes.c_int * 8)(9, 61, 9, 9, 9, 9, 9, 9)), E_ARG, b"bad dimensions"),       # the SECOND group is bad: nothing launched
    (dict(ld=20), E_ARG, b"row pitch"),
])
def test_shapelet_bwd_input_bank_validates_every_group_before_the_first_launch(kw, rc, msg):
    L = _lib_or_skip()
    assert L.ign_shapelet_bwd_input_bank(*_bank_args(**kw)) == rc
    assert msg in L.ign_last_error()


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(x=None), E_ARG, b"null pointer"),
    (dict(gx=None), E_ARG, b"null pointer"),
    (dict(T=1), E_ARG, b"T >= 2"),
    (dict(C=0), E_ARG, b"bad dimension"),
    (dict(T=50000), E_TOOBIG, b"LDS tile"),
])
def test_instnorm_bwd_argument_errors_need_no_device(kw, rc, msg):
    L = _lib_or_skip()
    a = dict(x=_p(16), g=_p(32), gx=_p(48), B=2, T=60, C=4, eps=1e-8, stream=None)
    a.update(kw)
    assert L.ign_instnorm_bwd(*a.values()) == rc
    assert msg in L.ign_last_error()


def test_saliency_refuses_models_without_a_shapelet_expert():
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from utils.saliency import input_saliency
    with pytest.raises(TypeError, match="shapelet expert"):
        input_saliency(torch.nn.Linear(3, 2), torch.zeros(1, 4, 3))
