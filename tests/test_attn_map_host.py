"""Attention map, host side: the C entry point ign_attn_probs (include/ign_abi.h "Attention map") is declared, bound and exported,
its argument errors come back before any launch, and FullAttention builds with output_attention=True while the mask still
raises.  The GPU side is tests/test_gpu_attn_map.py."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUP = -1001, -1002
F32, X6, BF16, H3 = 0, 1, 2, 3


def test_attn_probs_symbol_is_declared_bound_and_exported():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    assert re.search(r"\bign_attn_probs\s*\(", hdr)
    assert "ign_attn_probs" in _lib.SIGNATURES
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "ign_attn_probs")


def _args(**kw):
    """A well-formed argument list of ign_attn_probs (fake, aligned device pointers), with `kw` replacing single arguments."""
    a = dict(q=ctypes.c_void_p(16), k=ctypes.c_void_p(32), lse=ctypes.c_void_p(48), attn=ctypes.c_void_p(64), B=1, L=4, S=4, H=1,
             E=64, q_sb=256, q_sl=64, k_sb=256, k_sl=64, scale=0.125, stream=None, math=F32, bq=None, bk=None, p=0.1, seed=7)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(q=None), E_ARG, b"pointer"),
    (dict(k=None), E_ARG, b"pointer"),
    (dict(lse=None), E_ARG, b"pointer"),
    (dict(attn=None), E_ARG, b"pointer"),
    (dict(q=ctypes.c_void_p(20)), E_ARG, b"aligned"),
    (dict(B=0), E_ARG, b"dimensions"),
    (dict(S=-3), E_ARG, b"dimensions"),
    (dict(E=48), E_UNSUP, b"E=48"),
    (dict(E=8), E_UNSUP, b"E=8"),
    (dict(math=4), E_ARG, b"arithmetic"),
    (dict(math=-1), E_ARG, b"arithmetic"),
    (dict(math=BF16, E=128), E_UNSUP, b"bf16"),
    (dict(math=H3, E=128, bq=ctypes.c_void_p(16), bk=ctypes.c_void_p(16)), E_UNSUP, b"h3"),
    (dict(math=H3), E_ARG, b"bound"),
    (dict(math=H3, bq=ctypes.c_void_p(16)), E_ARG, b"bound"),
    (dict(q_sl=6), E_ARG, b"stride"),
    (dict(k_sb=0), E_ARG, b"stride"),
    (dict(p=1.0), E_ARG, b"p ="),
    (dict(p=-0.25), E_ARG, b"p ="),
    (dict(p=float("nan")), E_ARG, b"p ="),
    (dict(p=1.0 - 2.0 ** -18), E_ARG, b"keep rate"),
])
def test_attn_probs_argument_errors_need_no_device(kw, rc, msg):
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    L = _lib.lib()
    assert L.ign_attn_probs(*_args(**kw)) == rc
    assert msg in L.ign_last_error()


def test_full_attention_builds_with_output_attention_and_the_mask_still_raises():
    import speech_imagery_eeg_amd  # noqa: F401
    import torch
    from layers.SelfAttention_Family import FullAttention
    fa = FullAttention(False, output_attention=True)
    assert fa.output_attention and not fa.mask_flag
    x = torch.zeros(1, 4, 2, 16)
    with pytest.raises(NotImplementedError, match="mask"):
        FullAttention(True, output_attention=True)(x, x, x, None)
    with pytest.raises(NotImplementedError, match="mask"):
        FullAttention(True)(x, x, x, None)
