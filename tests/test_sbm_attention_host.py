"""SBM attention head, host side: the C entry points ign_sbm_attn_* (include/ign_abi.h) are declared, bound and exported, the
workspace size follows the documented O(B*F) layout, and argument errors come back before any launch.  The GPU side is
tests/test_gpu_sbm_attention.py."""
import ctypes
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUP = -1001, -1002
SYMBOLS = ("ign_sbm_attn_workspace_bytes", "ign_sbm_attn_fwd", "ign_sbm_attn_bwd")


def _lib_or_skip():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    return _lib.lib()


def test_sbm_attn_symbols_are_declared_bound_and_exported():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    h = ctypes.CDLL(_lib.lib_path())
    for name in SYMBOLS:
        assert hasattr(h, name), name


def test_sbm_attn_workspace_is_linear_in_batch_and_features():
    L = _lib_or_skip()
    assert L.ign_sbm_attn_workspace_bytes(0, 10) == 0
    assert L.ign_sbm_attn_workspace_bytes(4, 0) == 0
    for B, F in ((1, 1), (33, 31), (256, 2440), (256, 7320), (32, 19260)):
        nch = math.ceil(B / 32)
        floats = nch * F * (2 * 16 + 2) + nch * math.ceil(F / 64) + math.ceil(F / 16) * 64
        assert L.ign_sbm_attn_workspace_bytes(B, F) == 4 * floats, (B, F)
    assert L.ign_sbm_attn_workspace_bytes(256, 7320) < 8 << 20          # one (B,F,F) fp32 tensor here would be 55 GB


def _p(v):
    return ctypes.c_void_p(v)


def _fwd_args(**kw):
    a = dict(x=_p(16), ldx=64, wq=_p(32), bq=_p(48), wk=_p(64), bk=_p(80), pos=_p(96), out=_p(112), lse=None, B=2, F=64, D=16,
             scale=0.25, stream=None)
    a.update(kw)
    return list(a.values())


def _bwd_args(**kw):
    a = dict(x=_p(16), ldx=64, wq=_p(32), bq=_p(48), wk=_p(64), bk=_p(80), pos=_p(96), out=_p(112), lse=_p(128), gout=_p(144),
             gx=_p(160), gwq=_p(176), gbq=_p(192), gwk=_p(208), gbk=_p(224), gpos=_p(240), ws=_p(256), B=2, F=64, D=16, scale=0.25,
             stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(x=None), E_ARG, b"null pointer"),
    (dict(pos=None), E_ARG, b"null pointer"),
    (dict(wk=None), E_ARG, b"null pointer"),
    (dict(out=None), E_ARG, b"null pointer"),
    (dict(B=0), E_ARG, b"bad dimensions"),
    (dict(F=0), E_ARG, b"bad dimensions"),
    (dict(ldx=63), E_ARG, b"ldx"),
    (dict(scale=0.0), E_ARG, b"scale"),
    (dict(scale=float("nan")), E_ARG, b"scale"),
    (dict(D=8), E_UNSUP, b"D=8"),
])
def test_sbm_attn_fwd_argument_errors_need_no_device(kw, rc, msg):
    L = _lib_or_skip()
    assert L.ign_sbm_attn_fwd(*_fwd_args(**kw)) == rc
    assert msg in L.ign_last_error()


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(lse=None), E_ARG, b"null pointer"),
    (dict(gout=None), E_ARG, b"null pointer"),
    (dict(gpos=None), E_ARG, b"null pointer"),
    (dict(ws=None), E_ARG, b"workspace"),
    (dict(B=-1), E_ARG, b"bad dimensions"),
    (dict(ldx=1, F=2), E_ARG, b"ldx"),
    (dict(scale=float("inf")), E_ARG, b"scale"),
    (dict(D=32), E_UNSUP, b"D=32"),
])
def test_sbm_attn_bwd_argument_errors_need_no_device(kw, rc, msg):
    L = _lib_or_skip()
    assert L.ign_sbm_attn_bwd(*_bwd_args(**kw)) == rc
    assert msg in L.ign_last_error()


def test_selfattention_keeps_the_torch_composition_on_the_cpu():
    """CPU tensors take the torch composition (F.scaled_dot_product_attention), unchanged: same values as a restatement."""
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from models.Shapelet import SelfAttention
    torch.manual_seed(0)
    att = SelfAttention(12, 16)
    x = torch.rand(3, 12)
    pos = att.pos_embed.weight
    q = x[..., None] * att.q_proj.weight[:, 0] + att.q_proj.bias + pos
    k = x[..., None] * att.k_proj.weight[:, 0] + att.k_proj.bias + pos
    ref = torch.softmax(q @ k.transpose(1, 2) * 0.25, -1) @ x[..., None]
    torch.testing.assert_close(att(x), ref[..., 0], rtol=1e-5, atol=1e-6)
    assert set(att.state_dict()) == {"q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias", "pos_embed.weight"}
