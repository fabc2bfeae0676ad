"""ops.mix / ign_mix_btc on the GPU against the float32 numpy restatement of the rule (utils/mix.py:mix_reference), bitwise: odd and
dword-aligned-only rows, several blocks per sample, every lam and span edge, ragged lengths, the exact copy beside an infinite
partner, the padding, repeatability and the refusals.

Input: randn plus a per-channel offset in [-2, 2]; the padding of a ragged batch holds a sentinel, not zero, so a kernel that mixed
it would show."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SENTINEL = 777.0
# (5,37,3) odd T*C: rows are dword-aligned only, partial tail quad; (3,300,122) CHISCO's C, 36600 flat indices = 9 blocks per
# sample; (2,1,1) smallest; (1,50,4) a batch of one: roll = 0
SHAPES = [(5, 37, 3), (3, 300, 122), (2, 1, 1), (1, 50, 4)]
IDS = ["5x37x3", "3x300x122", "2x1x1", "1x50x4"]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import speech_imagery_eeg_amd  # noqa: F401
    return torch.device("cuda:0")


def _x(B, T, C):
    g = torch.Generator().manual_seed(1000 * B + 10 * T + C)
    return (torch.randn(B, T, C, generator=g) + (4 * torch.rand(C, generator=g) - 2)).contiguous()


def _lam(B, kind):
    g = np.random.default_rng(B)
    if kind == "edges":
        return np.resize(np.array([0.0, 1.0, 0.5], dtype=np.float32), B)
    return g.random(B, dtype=np.float32)


def _lens(B, T):
    """full, empty, and in between; sample b's partner under roll = 1 is b + 1: (T, short) is a partner shorter than the sample"""
    return np.resize(np.array([T, max(T // 3, 0), 0, T, max(T - 1, 0)], dtype=np.int32), B)


def _spans(B, n, kind):
    """m = 0, m = n, start = 0 and a span that ends at n, cycled over the samples"""
    n = np.asarray(n, dtype=np.int64)
    pick = {"none": [(0, 0)], "all": [(0, 1.0)], "edges": [(0, 0), (0, 1.0), (0, 0.5), (0.5, 1.0), (0.25, 0.5)]}[kind]
    out = np.zeros((B, 2), dtype=np.int32)
    for b in range(B):
        lo, hi = pick[b % len(pick)]
        s, e = int(lo * n[b]), int(round(hi * n[b]))
        out[b] = (s, e - s)
    return out


def _run(dev, x, lam, roll, span=None, lens=None):
    from ign_hip import ops
    xd = x.to(dev)
    put = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    out = ops.mix(xd, put(lam), roll, span=put(span), lengths=put(lens))
    assert out.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), x), "the input is left as it was"
    return out.cpu().numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def ref():
    import speech_imagery_eeg_amd  # noqa: F401
    from utils.mix import mix_reference
    return mix_reference


# ---------------------------------------------------------------- 1. bitwise against the restatement
@pytest.mark.parametrize("spans", ["none", "edges", "all"])
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("lam_kind", ["edges", "random"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_bitwise_equal_to_the_float32_restatement(ref, i, lam_kind, ragged, spans):
    dev = _dev()
    B, T, C = SHAPES[i]
    x = _x(B, T, C)
    lens = _lens(B, T) if ragged else None
    if ragged:
        for b, n in enumerate(lens):
            x[b, n:] = SENTINEL
    lam = _lam(B, lam_kind)
    span = None if spans == "none" else _spans(B, lens if ragged else np.full(B, T), spans)
    for roll in sorted({1, B - 1} if B > 1 else {0}):
        out = _run(dev, x, lam, roll, span, lens)
        assert _same_bits(out, ref(x.numpy(), lens, roll, lam, span)), roll
        if ragged:
            for b, n in enumerate(lens):
                assert (out[b, n:] == SENTINEL).all()                  # padding is copied through, never mixed
        if B == 1 and spans == "none" and lam_kind == "edges":
            assert lam[0] == 0.0 and np.array_equal(out, x.numpy())    # roll = 0: 0 * x + 1 * x
    if B > 1 and T * C > 64 and not ragged:
        assert not np.array_equal(out, x.numpy())                      # the case exercises something


def test_no_lengths_equal_full_lengths_and_no_span_equals_empty_spans(ref):
    dev = _dev()
    for B, T, C in SHAPES[:2]:
        x, lam = _x(B, T, C), _lam(B, "random")
        span = _spans(B, np.full(B, T), "edges")
        a = _run(dev, x, lam, 1, span, None)
        assert _same_bits(a, _run(dev, x, lam, 1, span, np.full(B, T, dtype=np.int32)))
        b = _run(dev, x, lam, 1, None, None)
        assert _same_bits(b, _run(dev, x, lam, 1, np.zeros((B, 2), dtype=np.int32), None))


def test_spans_and_lengths_out_of_range_are_clamped(ref):
    """device data is never trusted as an index bound: the kernel and the restatement clamp alike"""
    dev = _dev()
    B, T, C = 5, 37, 3
    x, lam = _x(B, T, C), _lam(B, "random")
    lens = np.array([T + 5, -3, 10, T, 2 ** 31 - 1], dtype=np.int32)
    span = np.array([[-4, 10], [0, 5], [8, 2 ** 31 - 1], [2 ** 31 - 1, 2 ** 31 - 1], [30, -1]], dtype=np.int32)
    assert _same_bits(_run(dev, x, lam, 2, span, lens), ref(x.numpy(), lens, 2, lam, span))


# ---------------------------------------------------------------- 2. the exact copy
def test_lam_one_is_a_bitwise_copy_beside_an_infinite_partner(ref):
    dev = _dev()
    B, T, C = 3, 300, 122
    x = _x(B, T, C)
    x[1] = float("inf")                                                # the partner of row 0 under roll = 1
    lam = np.array([1.0, 1.0, 0.5], dtype=np.float32)
    out = _run(dev, x, lam, 1)
    assert _same_bits(out[0], x[0].numpy()) and np.isfinite(out[0]).all()
    assert _same_bits(out[1], x[1].numpy())
    assert _same_bits(out, ref(x.numpy(), None, 1, lam, None))
    # with a span the rest of a lam = 1 row is still a copy; the span takes the partner as it is
    span = np.array([[10, 20], [0, 0], [0, 0]], dtype=np.int32)
    out = _run(dev, x, lam, 1, span)
    assert np.isinf(out[0, 10:30]).all() and _same_bits(out[0, :10], x[0, :10].numpy()) and _same_bits(out[0, 30:], x[0, 30:].numpy())


# ---------------------------------------------------------------- 3. repeatability
def test_two_calls_are_bitwise_equal():
    dev = _dev()
    B, T, C = 3, 300, 122
    x, lam = _x(B, T, C), _lam(B, "random")
    span, lens = _spans(B, _lens(B, T), "edges"), _lens(B, T)
    assert _same_bits(_run(dev, x, lam, 2, span, lens), _run(dev, x, lam, 2, span, lens))


# ---------------------------------------------------------------- 4. refusals
def test_refusals():
    dev = _dev()
    from ign_hip import _lib, ops
    x = torch.randn(2, 8, 3, device=dev)
    lam = torch.full((2,), 0.5, device=dev)
    with pytest.raises(_lib.IgnError, match="requires a gradient"):
        ops.mix(x.clone().requires_grad_(True), lam, 1)
    with pytest.raises(_lib.IgnError, match="contiguous"):
        ops.mix(x.permute(0, 2, 1), lam, 1)
    with pytest.raises(_lib.IgnError, match="float32"):
        ops.mix(x.double(), lam, 1)
    with pytest.raises(_lib.IgnError, match="float32"):
        ops.mix(x, lam.double(), 1)
    with pytest.raises(_lib.IgnError):
        ops.mix(x.cpu(), lam, 1)
    with pytest.raises(_lib.IgnError):
        ops.mix(x, lam.cpu(), 1)
    with pytest.raises(_lib.IgnError, match="lam"):
        ops.mix(x, lam[:1], 1)
    with pytest.raises(_lib.IgnError, match="lengths"):
        ops.mix(x, lam, 1, lengths=torch.tensor([8, 8], device=dev))                  # int64
    with pytest.raises(_lib.IgnError, match="span"):
        ops.mix(x, lam, 1, span=torch.zeros(2, 2, device=dev))                        # float32
    with pytest.raises(_lib.IgnError, match="span"):
        ops.mix(x, lam, 1, span=torch.zeros(2, dtype=torch.int32, device=dev))
    for roll in (2, -1):
        with pytest.raises(_lib.IgnError, match="roll"):
            ops.mix(x, lam, roll)


def test_c_abi_refuses_in_place_and_a_bad_roll():
    dev = _dev()
    from ign_hip import _lib
    L = _lib.lib()
    x = torch.randn(2, 8, 3, device=dev)
    keep = x.clone()
    out = torch.full_like(x, 5.0)
    lam = torch.full((2,), 0.5, device=dev)
    p, q, l = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(lam.data_ptr())

    def call(src, dst, lam=l, roll=1, B=2, T=8, C=3):
        return L.ign_mix_btc(src, dst, None, lam, None, roll, B, T, C, _lib.stream())
    assert call(p, p) == -1001                                                          # IGN_E_ARG
    msg = L.ign_last_error().decode()
    assert "ign_mix_btc" in msg and "overlap" in msg
    assert call(p, ctypes.c_void_p(x.data_ptr() + 4 * 24)) == -1001                     # out begins at x's second sample
    for kw in (dict(roll=2), dict(roll=-1), dict(T=0), dict(B=0), dict(C=0), dict(lam=None)):
        assert call(p, q, **kw) == -1001, kw
    assert call(None, q) == -1001 and call(p, None) == -1001
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and bool((out == 5.0).all())                            # nothing was launched


def test_may_be_captured():
    """every argument but roll is device data: a replay mixes what the static inputs hold then"""
    dev = _dev()
    from ign_hip import ops
    from utils.mix import mix_reference
    x, lam = _x(5, 37, 3).to(dev), torch.from_numpy(_lam(5, "random")).to(dev)
    ops.mix(x, lam, 2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.mix(x, lam, 2)
    x.copy_(_x(5, 37, 3).flip(0).to(dev))
    lam.fill_(0.25)
    g.replay()
    torch.cuda.synchronize()
    assert _same_bits(out.cpu().numpy(), mix_reference(x.cpu().numpy(), None, 2, lam.cpu().numpy(), None))
