"""Attention dropout, host side: the numpy restatement of the keep mask (csrc/ign_dropout.h, include/ign_abi.h "Attention dropout")
against the Random123 known-answer vectors, the threshold / scale rule, the Python surface's argument handling and the new C ABI
symbols.  The GPU tests (test_gpu_attn_dropout.py) compare the kernels' masks with `keep_mask` below bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Random123) on arrays: ctr = 4 broadcastable uint32-valued arrays, key = (k0, k1) -> 4 uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _U32 for x in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _U32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def dropout_threshold(p):
    """thr = round(p * 65536) with p as the fp32 the kernels receive (round half to even), s = 65536 / (65536 - thr) in fp32."""
    thr = int(np.rint(np.float64(np.float32(p)) * 65536.0))
    return thr, np.float32(np.float32(65536.0) / np.float32(65536 - thr))


def keep_mask(B, H, L, S, p, seed):
    """(B, H, L, S) bool keep mask of one call: element (b, h, i, j) reads halfword n = (i & 3) * 4 + (j & 3) of the 4 x 4 block
    (i >> 2, j >> 2); call n >> 3 has counter (i >> 2, j >> 2, b * H + h, n >> 3) under key (seed low word, seed high word)."""
    thr, _ = dropout_threshold(p)
    i = np.arange(L, dtype=np.uint64)[:, None]
    j = np.arange(S, dtype=np.uint64)[None, :]
    n = (i & np.uint64(3)) * np.uint64(4) + (j & np.uint64(3))
    call = n >> np.uint64(3)
    word = (n & np.uint64(7)) >> np.uint64(1)
    half = n & np.uint64(1)
    out = np.empty((B, H, L, S), dtype=bool)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    for b in range(B):
        for h in range(H):
            x = philox4x32_10((i >> np.uint64(2), j >> np.uint64(2), np.uint64(b * H + h), call), key)
            w = np.choose(word.astype(np.int64), [t.astype(np.uint64) for t in x])
            u16 = (w >> (half * np.uint64(16))) & np.uint64(0xFFFF)
            out[b, h] = u16 >= np.uint64(thr)
    return out


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_restatement_reproduces_random123_known_answers(ctr, key, want):
    got = tuple(int(x) for x in philox4x32_10(ctr, key))
    assert got == want, [hex(x) for x in got]


@pytest.mark.parametrize("p,thr,scale", [(0.05, 3277, 65536.0 / 62259.0), (0.1, 6554, 65536.0 / 58982.0), (0.5, 32768, 2.0)])
def test_threshold_and_scale_of_the_documented_rule(p, thr, scale):
    t, s = dropout_threshold(p)
    assert t == thr
    assert s == np.float32(scale)
    assert abs(t / 65536.0 - p) <= 2.0 ** -17                        # the rate actually used is within 2^-17 of p
    from_ops = _ops_threshold(p)
    if from_ops is not None:
        assert from_ops == (t, float(s))


def _ops_threshold(p):
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    return ops.dropout_threshold(p)


def test_keep_mask_blocks_are_pure_functions_of_the_element():
    """The mask of a sub-rectangle equals that rectangle of a larger call's mask (no dependence on the shape), and the helper
    layouts agree: one Philox call serves 4 consecutive keys of a query."""
    big = keep_mask(2, 3, 40, 50, 0.3, 0x123456789ABCDEF)
    small = keep_mask(2, 3, 13, 21, 0.3, 0x123456789ABCDEF)
    assert np.array_equal(big[:, :, :13, :21], small)
    assert not np.array_equal(keep_mask(1, 1, 16, 16, 0.3, 1), keep_mask(1, 1, 16, 16, 0.3, 2))
    assert keep_mask(1, 2, 8, 8, 0.0, 5).all()
    frac = keep_mask(2, 4, 128, 128, 0.25, 99).mean()
    assert abs(frac - 0.75) < 5 * np.sqrt(0.25 * 0.75 / (2 * 4 * 128 * 128))


def test_dropout_argument_checks_need_no_device():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops, _lib
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.dropout_threshold(bad)
    with pytest.raises(ValueError):
        ops.dropout_threshold(1.0 - 2.0 ** -18)                       # rounds to thr = 65536: nothing would be kept
    path = _lib.lib_path()
    if not os.path.exists(path):
        pytest.skip("libign_hip.so not built")
    L = _lib.lib()
    # p outside [0, 1) and unsupported E are rejected before any device work
    assert L.ign_attn_dropout_mask(None, 1, 1, 4, 4, 0.1, 1, None) == -1001
    assert L.ign_attn_dropout_mask(ctypes.c_void_p(16), 1, 1, 4, 4, 1.0, 1, None) == -1001
    assert b"p =" in L.ign_last_error()
    args = [ctypes.c_void_p(16)] * 5 + [1, 4, 4, 1, 64] + [64] * 6 + [0.125, None, 0, None, None, None]
    assert L.ign_attn_fwd_dropout(*args, -0.5, 7) == -1001
    args[9] = 48
    assert L.ign_attn_fwd_dropout(*args, 0.1, 7) == -1002
    args[9] = 64
    assert L.ign_attn_fwd_dropout(*args[:16], 0.125, None, 9, None, None, None, 0.1, 7) == -1001     # unknown arithmetic


def test_new_dropout_symbols_are_declared_bound_and_exported():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    names = ("ign_attn_fwd_dropout", "ign_attn_bwd_dropout", "ign_attn_dropout_mask")
    for n in names:
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert n in _lib.SIGNATURES, n
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    h = ctypes.CDLL(_lib.lib_path())
    for n in names:
        assert hasattr(h, n), n


# (ATTN_MATH, GEMM_MATH, autocast) -> the attention arithmetic at E = 16, 32, 64, 128: (forward, backward)
_ARITH_TABLE = {
    ("bf16x6", "f16x3", False): ("H3 H3 H3 X6", "H3 H3 H3 F32"),
    ("bf16x6", "f16x3", True): ("BF16 BF16 BF16 X6", "BF16 BF16 BF16 F32"),
    ("bf16x6", "bf16x6", False): ("X6 X6 X6 X6", "X6 X6 X6 F32"),
    ("bf16x6", "bf16x6", True): ("BF16 BF16 BF16 X6", "BF16 BF16 BF16 F32"),
    ("f32", "f16x3", False): ("F32 F32 F32 F32", "F32 F32 F32 F32"),
    ("f32", "f16x3", True): ("BF16 BF16 BF16 F32", "BF16 BF16 BF16 F32"),
    ("f32", "bf16x6", False): ("F32 F32 F32 F32", "F32 F32 F32 F32"),
    ("f32", "bf16x6", True): ("BF16 BF16 BF16 F32", "BF16 BF16 BF16 F32"),
}


def test_attention_arithmetic_rule_and_packed_fallback(monkeypatch):
    """ops._attn_arith, the one statement of which attention kernels run, against the table above; and attention_packed takes
    the unpacked path exactly for ATTN_MATH != "bf16x6" or E > 64 (there the CPU tensor reaches the monkeypatched `attention`;
    the packed path refuses it before any launch)."""
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops, _lib
    monkeypatch.setattr(ops, "attention", lambda *a: "unpacked")
    for (attn_math, gemm_math, autocast), rows in _ARITH_TABLE.items():
        monkeypatch.setattr(ops, "ATTN_MATH", attn_math)
        monkeypatch.setattr(ops, "GEMM_MATH", gemm_math)
        for bwd, row in enumerate(rows):
            for E, want in zip((16, 32, 64, 128), row.split()):
                got = ops._attn_arith(E, autocast, bool(bwd))
                assert got == getattr(ops, "ATTN_MATH_" + want), (attn_math, gemm_math, autocast, E, bwd, want, got)
        for E in (16, 32, 64, 128):
            qkv = torch.zeros(1, 4, 3, 1, E)
            if attn_math != "bf16x6" or E > 64:
                assert ops.attention_packed(qkv, 1.0) == "unpacked"
            else:
                with pytest.raises(_lib.IgnError, match="no CPU fallback"):
                    ops.attention_packed(qkv, 1.0)
