"""SBM bilinear head, host side: the C entry points ign_sbm_bilinear_* (include/ign_abi.h) are declared, bound and exported,
the workspace is the documented O(B*N*F) layout (never F*F), argument errors come back before any launch, and a
CPU model keeps nn.Bilinear.  The GPU side is tests/test_gpu_sbm_bilinear.py."""
import ctypes
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1001
SYMBOLS = ("ign_sbm_bilinear_workspace_bytes", "ign_sbm_bilinear_fwd", "ign_sbm_bilinear_bwd")


def _lib_or_skip():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    return _lib.lib()


def test_sbm_bilinear_symbols_are_declared_bound_and_exported():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ops
    assert callable(getattr(ops, "sbm_bilinear", None))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    h = ctypes.CDLL(_lib.lib_path())
    for name in SYMBOLS:
        assert hasattr(h, name), name


def test_sbm_bilinear_workspace_is_linear_in_batch_classes_and_features():
    L = _lib_or_skip()
    assert L.ign_sbm_bilinear_workspace_bytes(0, 10, 3) == 0
    assert L.ign_sbm_bilinear_workspace_bytes(4, 0, 3) == 0
    assert L.ign_sbm_bilinear_workspace_bytes(4, 10, 0) == 0
    for B, F, N in ((1, 1, 1), (3, 72, 4), (8, 130, 3), (32, 360, 4), (256, 2440, 3), (256, 7320, 3)):
        fwd = B * N * math.ceil(F / 128)                  # forward: partial row dots per 128-column tile
        bwd = B * N * F if N > 1 else 0                    # backward: per-class partials of gu
        assert L.ign_sbm_bilinear_workspace_bytes(B, F, N) == 4 * max(fwd, bwd), (B, F, N)
    assert L.ign_sbm_bilinear_workspace_bytes(256, 7320, 3) == 4 * 256 * 3 * 7320   # 22.5 MB; one (B,F,F) tensor is 55 GB
    assert L.ign_sbm_bilinear_workspace_bytes(32, 100000, 1) == 4 * 32 * math.ceil(100000 / 128)


def _p(v):
    return ctypes.c_void_p(v)


def _fwd_args(**kw):
    a = dict(u=_p(16), v=_p(32), w=_p(48), out=_p(64), t=None, ws=_p(80), B=2, F=64, N=3, stream=None)
    a.update(kw)
    return list(a.values())


def _bwd_args(**kw):
    a = dict(u=_p(16), v=_p(32), w=_p(48), t=_p(64), gout=_p(80), gu=_p(96), gv=_p(112), gw=_p(128), ws=_p(144), B=2, F=64, N=3,
             stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw,msg", [
    (dict(u=None), b"null pointer"),
    (dict(v=None), b"null pointer"),
    (dict(w=None), b"null pointer"),
    (dict(out=None), b"null pointer"),
    (dict(ws=None), b"workspace"),
    (dict(B=0), b"bad dimensions"),
    (dict(F=-1), b"bad dimensions"),
    (dict(N=0), b"bad dimensions"),
    (dict(F=1 << 30), b"grid too large"),
])
def test_sbm_bilinear_fwd_argument_errors_need_no_device(kw, msg):
    L = _lib_or_skip()
    assert L.ign_sbm_bilinear_fwd(*_fwd_args(**kw)) == E_ARG
    assert msg in L.ign_last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(u=None), b"null pointer"),
    (dict(w=None), b"null pointer"),
    (dict(gout=None), b"gout"),
    (dict(t=None), b"t_save"),
    (dict(ws=None), b"workspace"),
    (dict(B=-1), b"bad dimensions"),
    (dict(N=0), b"bad dimensions"),
])
def test_sbm_bilinear_bwd_argument_errors_need_no_device(kw, msg):
    L = _lib_or_skip()
    assert L.ign_sbm_bilinear_bwd(*_bwd_args(**kw)) == E_ARG
    assert msg in L.ign_last_error()


def test_cpu_model_keeps_nn_bilinear():
    """CPU tensors take nn.Bilinear, unchanged: head() equals output_layer + output_bilinear and the state_dict keys stay."""
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from conftest import make_cfg
    from models.Shapelet import ShapeBottleneckModel
    torch.manual_seed(0)
    m = ShapeBottleneckModel(make_cfg(sbm_cls="bilinear"), [2, 3], [0.1, 0.3])
    assert isinstance(m.output_bilinear, torch.nn.Bilinear) and m.output_bilinear.bias is None
    assert "output_bilinear.weight" in m.state_dict() and tuple(m.output_bilinear.weight.shape) == (4, 30, 30)
    p = torch.rand(5, 30)
    ref = m.output_layer(p) + torch.einsum("bi,nij,bj->bn", p, m.output_bilinear.weight, p)
    torch.testing.assert_close(m.head(p), ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(m.head(p), m.output_layer(p) + m.output_bilinear(p, p), rtol=0, atol=0)
