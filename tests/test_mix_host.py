"""--mix on the host (no GPU): the flag's parser, the per-step draws (utils.mix.mix_draws: repeatability, ranges, the CutMix share, the
statistics of lam at ONE fixed seed), the float64 restatement of the soft-label criterion against F.cross_entropy and float64
autograd, the numpy restatement of the batch rule at its edges, which entry point ops.ign_loss reaches with soft labels (against a
recording stand-in library), and the two new symbols in header / bindings / library.  The GPU side is tests/test_gpu_mix*.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

import speech_imagery_eeg_amd  # noqa: F401
from utils import mix as M
from utils.augment import step_seed

SEED = 0x5EED0A06C0FFEE11
MIX, LOSS = "ign_mix_btc", "ign_loss_mix_fwd_bwd_reg"


# ---------------------------------------------------------------- parser
def test_parse_accepts():
    assert M.parse_mix("none") == M.MixSpec() and not M.parse_mix("none").active
    assert M.parse_mix("") == M.MixSpec() and M.parse_mix(None) == M.MixSpec()
    assert M.parse_mix("mixup=0.4") == M.MixSpec(mixup=0.4, cutmix=0.0, prob=1.0) and M.parse_mix("mixup=0.4").active
    assert M.parse_mix("cutmix=1,prob=0.5") == M.MixSpec(cutmix=1.0, prob=0.5)
    s = M.parse_mix(" cutmix=1 , mixup=0.4,prob=1")
    assert s == M.MixSpec(mixup=0.4, cutmix=1.0, prob=1.0) and M.parse_mix(s) is s


@pytest.mark.parametrize("bad", ["mixup=0", "mixup=-1", "cutmix=0", "mixup=inf", "mixup=nan", "mixup=0.4,prob=0", "mixup=0.4,prob=1.5",
                                 "mixup=0.4,prob=-0.1", "mixup=0.4,prob=nan", "shift=0.1", "mixup", "mixup=", "mixup=abc",
                                 "mixup=0.4,mixup=0.5", "mixup=0.4;cutmix=1", "prob=0.5", "balanced"])
def test_parse_rejects(bad):
    with pytest.raises(ValueError):
        M.parse_mix(bad)


def test_flag():
    import run
    p = run.build_parser()
    act = {a.option_strings[0]: a for a in p._actions if a.option_strings}["--mix"]
    assert act.default == "none" and act.help
    assert "--mix" in run.__doc__
    a = run.get_args(["--data", "SYNTH", "--mix", "mixup=0.4,cutmix=1"])
    assert M.parse_mix(a.mix) == M.MixSpec(mixup=0.4, cutmix=1.0)
    with pytest.raises(ValueError):
        run.get_args(["--data", "SYNTH", "--mix", "mixup=0"])
    with pytest.raises(ValueError, match="regression"):
        run.get_args(["--data", "SYNTH", "--task_name", "regression", "--mix", "mixup=0.4"])
    run.get_args(["--data", "SYNTH", "--task_name", "regression", "--mix", "none"])
    with pytest.raises(ValueError):                                   # --augment keeps refusing the key (the flag is its own)
        run.get_args(["--data", "SYNTH", "--augment", "mixup=0.1"])


# ---------------------------------------------------------------- draws
BOTH = M.MixSpec(mixup=0.4, cutmix=1.0)


def test_draws_repeat_and_depend_on_the_seed():
    lens = np.arange(64) % 41
    a, b = M.mix_draws(SEED, 64, lens, BOTH), M.mix_draws(SEED, 64, lens, BOTH)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[1].dtype == np.float32 and a[1].shape == (64,) and a[2].dtype == np.int32 and a[2].shape == (64, 2)
    c = M.mix_draws(SEED ^ 1, 64, lens, BOTH)
    assert not np.array_equal(a[1], c[1]) and not np.array_equal(a[2], c[2])
    # the per-step seed of --augment: ranks and steps differ, the same (rank, step) repeats
    r0, r1 = M.mix_draws(step_seed(7, 0, 3), 64, lens, BOTH), M.mix_draws(step_seed(7, 1, 3), 64, lens, BOTH)
    assert not np.array_equal(r0[1], r1[1])
    assert np.array_equal(r0[1], M.mix_draws(step_seed(7, 0, 3), 64, lens, BOTH)[1])
    # no global generator is consumed
    st, tst = np.random.get_state()[1].copy(), torch.get_rng_state()
    M.mix_draws(SEED, 64, lens, BOTH)
    assert np.array_equal(np.random.get_state()[1], st) and torch.equal(torch.get_rng_state(), tst)


def test_roll_is_a_pairing_without_self_pairs():
    assert M.mix_draws(SEED, 1, 10, BOTH)[0] == 0
    seen = set()
    for s in range(200):
        for B in (2, 3, 5, 64):
            roll = M.mix_draws(step_seed(1, 0, s), B, 10, BOTH)[0]
            assert isinstance(roll, int) and 1 <= roll < B
            if B == 5:
                seen.add(roll)
    assert seen == {1, 2, 3, 4}


def test_ranges_spans_and_the_cutmix_share():
    B = 4096
    lens = np.arange(B) % 34                                           # n = 0 .. 33
    roll, lam, span = M.mix_draws(SEED, B, lens, BOTH)
    start, m = span[:, 0].astype(np.int64), span[:, 1].astype(np.int64)
    assert (lam >= 0).all() and (lam <= 1).all()
    assert (start >= 0).all() and (m >= 0).all() and (start + m <= lens).all()
    cut = m > 0
    assert cut.sum() > B // 4 and (~cut).sum() > B // 4                # both kinds occur
    assert np.array_equal(lam[cut], (1.0 - m[cut] / lens[cut]).astype(np.float32))       # exactly the share that is kept
    assert (span[~cut] == 0).all()                                     # mixup and unmixed samples: the empty span (0, 0)
    assert (lam[lens == 0] == 1).all() and (span[lens == 0] == 0).all()
    # cutmix alone: every sample is a CutMix sample (lam is a multiple of 1/n); mixup alone: no spans at all
    _, lam_c, span_c = M.mix_draws(SEED, B, np.full(B, 20), M.MixSpec(cutmix=1.0))
    assert np.array_equal(lam_c, (1.0 - span_c[:, 1] / 20.0).astype(np.float32))
    assert set(span_c[:, 1].tolist()) == set(range(21))                # lam' uniform at A = 1: every span length, none and all too
    assert span_c[:, 0].min() == 0 and (span_c.sum(1) == 20).any()     # spans that start at 0 and spans that end at n
    _, lam_m, span_m = M.mix_draws(SEED, B, np.full(B, 20), M.MixSpec(mixup=0.4))
    assert (span_m == 0).all() and len(np.unique(lam_m)) > B // 2
    assert np.array_equal(lam_m, M.mix_draws(SEED, B, 20, M.MixSpec(mixup=0.4))[1])      # one length for all
    with pytest.raises(ValueError):
        M.mix_draws(SEED, 2, [3, -1], BOTH)


def test_prob_leaves_unmixed_rows():
    B = 4096
    _, lam, span = M.mix_draws(SEED, B, 50, M.MixSpec(mixup=0.4, cutmix=1.0, prob=0.25))
    plain = (lam == 1) & (span[:, 1] == 0)
    # lam == 1 by chance needs Beta(0.4, 0.4) to round to 1 in float32 (~1e-3 of the draws) or a CutMix span of 0 / 50 (1%)
    assert abs(plain.mean() - 0.75) <= 6 * np.sqrt(0.75 * 0.25 / B) + 0.01
    _, lam1, _ = M.mix_draws(SEED, B, 50, M.MixSpec(mixup=0.4))
    assert (lam1 == 1).mean() < 0.01


def test_lam_statistics_of_mixup():
    """20000 draws at A = 0.4: the mean of lam is 0.5 within 0.01 (the standard deviation of Beta(0.4, 0.4) is 0.373: 0.01 is
    3.8 standard errors -- checked for this seed, a condition on a correct generator, not a measurement) and the distribution is
    symmetric about 0.5: as many draws below as above (6 standard errors), and the quantiles mirror each other."""
    n = 20000
    _, lam, _ = M.mix_draws(SEED, n, 100, M.MixSpec(mixup=0.4))
    lam = lam.astype(np.float64)
    assert abs(lam.mean() - 0.5) <= 0.01
    assert abs((lam < 0.5).mean() - 0.5) <= 6 * 0.5 / np.sqrt(n)
    q = np.quantile(lam, [0.05, 0.1, 0.25, 0.4])
    assert np.abs(q + np.quantile(lam, [0.95, 0.9, 0.75, 0.6]) - 1.0).max() <= 0.02
    assert abs(lam.var() - 1.0 / (4 * (2 * 0.4 + 1))) <= 0.01           # Beta(A, A): 1 / (4 (2A + 1)) = 0.1389


# ---------------------------------------------------------------- the batch rule in numpy
def test_mix_reference_edges():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((4, 6, 2)).astype(np.float32)
    x[1] = np.inf                                                      # the partner of row 0 under roll = 1
    lam = np.array([1.0, 0.0, 0.5, 0.25], dtype=np.float32)
    span = np.array([[0, 0], [0, 0], [2, 3], [0, 6]], dtype=np.int32)
    lens = np.array([6, 6, 6, 4])
    out = M.mix_reference(x, lens, 1, lam, span)
    assert out.dtype == np.float32 and np.array_equal(out[0], x[0])                    # lam = 1: a copy, no NaN from 0 * inf
    assert np.array_equal(out[2, 2:5], x[3, 2:5]) and np.array_equal(out[2, :2], np.float32(0.5) * x[2, :2] + np.float32(0.5) * x[3, :2])
    assert np.array_equal(out[3, :4], x[0, :4]) and np.array_equal(out[3, 4:], x[3, 4:])   # the span is clamped to n; padding kept
    assert np.array_equal(M.mix_reference(x[2:], None, 0, lam[2:], None)[0], np.float32(0.5) * x[2] + np.float32(0.5) * x[2])
    full = M.mix_reference(x, None, 3, lam, None)
    assert np.array_equal(full[2], np.float32(0.5) * x[2] + np.float32(0.5) * x[1])    # p = (2 + 3) mod 4


# ---------------------------------------------------------------- the criterion in float64
def _ce_case(B=9, N=5):
    g = torch.Generator().manual_seed(11)
    z = (torch.randn(B, N, generator=g) * 3).double()
    ya, yb = torch.randint(0, N, (B,), generator=g), torch.randint(0, N, (B,), generator=g)
    lam = torch.rand(B, generator=g).double()
    lam[0], lam[1] = 0.0, 1.0
    w = (0.2 + 4.8 * torch.rand(N, generator=g)).double()
    return z, ya, yb, lam, w


@pytest.mark.parametrize("weights,eps", [(False, 0.0), (True, 0.0), (True, 0.1), (False, 0.1)])
def test_reference_reduces_to_cross_entropy(weights, eps):
    z, ya, yb, lam, w = _ce_case()
    w = w if weights else None
    wn = None if w is None else w.numpy()
    want = float(F.cross_entropy(z, ya, weight=w, label_smoothing=eps))
    got = M.mix_cross_entropy_reference(z.numpy(), ya.numpy(), yb.numpy(), np.ones(len(ya)), wn, eps)
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want))
    # ya == yb: lam does not matter
    same = M.mix_cross_entropy_reference(z.numpy(), ya.numpy(), ya.numpy(), lam.numpy(), wn, eps)
    assert abs(same - want) <= 1e-12 * max(1.0, abs(want))
    if w is None and eps == 0.0:                                       # the usual mixup loss
        usual = (lam * F.cross_entropy(z, ya, reduction='none') + (1 - lam) * F.cross_entropy(z, yb, reduction='none')).mean()
        got = M.mix_cross_entropy_reference(z.numpy(), ya.numpy(), yb.numpy(), lam.numpy())
        assert abs(got - float(usual)) <= 1e-12


@pytest.mark.parametrize("weights,eps", [(False, 0.0), (True, 0.1)])
def test_reference_gradient_and_torch_composition_agree_with_float64_autograd(weights, eps):
    z, ya, yb, lam, w = _ce_case()
    w = w if weights else None
    zt = z.clone().requires_grad_(True)
    loss = M.mix_cross_entropy(zt, ya, yb, lam, w, eps)
    assert loss.dtype == torch.float32                                 # the composition is fp32 whatever it is given
    z64 = z.clone().requires_grad_(True)
    lp = torch.log_softmax(z64, -1)
    wv = torch.ones(z.shape[1], dtype=torch.float64) if w is None else w
    a, c = lam * wv[ya], (1 - lam) * wv[yb]
    rows = torch.arange(len(ya))
    l64 = ((1 - eps) * (a * -lp[rows, ya] + c * -lp[rows, yb]).sum() + eps / z.shape[1] * (-lp * wv).sum()) / (a + c).sum()
    l64.backward()
    l64 = l64.detach()
    got, grad = M.mix_cross_entropy_reference(z.numpy(), ya.numpy(), yb.numpy(), lam.numpy(), None if w is None else w.numpy(), eps,
                                              grad=True)
    assert abs(got - float(l64)) <= 1e-12 * max(1.0, abs(float(l64)))
    assert np.abs(grad - z64.grad.numpy()).max() <= 1e-12
    loss.backward()
    assert abs(float(loss) - float(l64)) <= 1e-5 * max(1.0, abs(float(l64)))
    assert float((zt.grad - z64.grad).abs().max()) <= 1e-5 * float(z64.grad.abs().max())


# ---------------------------------------------------------------- which entry point
class _StandIn:
    """Every attribute is an entry point that records (name, args) and answers 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _header_params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
    assert m, name
    return [re.split(r"[\s*]+", p.strip())[-1] for p in m.group(1).split(",")]


def test_soft_labels_reach_the_new_entry_point(monkeypatch):
    from ign_hip import _lib, ops
    rec = _StandIn()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "check", lambda rc, what: None)
    monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(0x5EED))
    monkeypatch.setattr(ops, "_need_gpu", lambda name, *ts: None)
    B, N = 5, 7
    g = torch.Generator().manual_seed(3)
    s, d = torch.randn(B, N, generator=g).requires_grad_(True), torch.randn(B, N, generator=g).requires_grad_(True)
    y, yb, lam = torch.arange(B) % N, (torch.arange(B) + 2) % N, torch.rand(B, generator=g)
    w = torch.linspace(0.5, 2.0, N)
    reg = torch.full((1,), 0.25, requires_grad=True)
    loss, out, eta = ops.ign_loss(s, d, y, 0.75, reg=reg, class_weight=w, label_smoothing=0.1, y_b=yb, lam=lam)
    (call,) = rec.calls
    name, args = call
    params = _header_params(LOSS)
    assert name == LOSS and len(args) == len(_lib.SIGNATURES[LOSS][1]) == len(params)
    got = dict(zip(params, (a.value if isinstance(a, ctypes.c_void_p) else a for a in args)))
    assert (got["B"], got["N"], got["beta"], got["stream"]) == (B, N, 0.75, 0x5EED) and got["label_smoothing"] == pytest.approx(0.1)
    assert got["labels"] == y.data_ptr() and got["labels_b"] == yb.data_ptr() and got["lam_b"] == lam.data_ptr()
    assert got["class_w"] == w.data_ptr() and got["reg"] == reg.data_ptr() and got["gdnn"] - got["gsbm"] == 4 * B * N
    assert loss.data_ptr() == got["loss3"] + 8 and loss.requires_grad and not out.requires_grad
    del rec.calls[:]
    loss.backward()                                                    # nine inputs, gradients for sbm / dnn / reg only; no launch
    assert s.grad.shape == (B, N) and d.grad.shape == (B, N) and reg.grad.shape == (1,) and not rec.calls
    # without class weights the pointer is null; without soft labels the call is the entry point it always was
    ops.ign_loss(s, d, y, 0.75, y_b=yb, lam=lam)
    assert rec.calls[-1][0] == LOSS and dict(zip(params, rec.calls[-1][1]))["class_w"] is None
    ops.ign_loss(s, d, y, 0.75)
    assert rec.calls[-1][0] == "ign_loss_fwd_bwd_reg"
    ops.ign_loss(s, d, y, 0.75, class_weight=w)
    assert rec.calls[-1][0] == "ign_loss_w_fwd_bwd_reg"
    n = len(rec.calls)
    for kw in (dict(y_b=yb), dict(lam=lam), dict(y_b=yb, lam=lam.double()), dict(y_b=yb, lam=lam[:-1]), dict(y_b=yb[:-1], lam=lam),
               dict(y_b=yb.float(), lam=lam), dict(y_b=yb, lam=lam.clone().requires_grad_(True)),
               dict(y_b=yb, lam=lam, label_smoothing=1.0)):
        with pytest.raises(_lib.IgnError):
            ops.ign_loss(s, d, y, 0.75, **kw)
    assert len(rec.calls) == n                                         # refusals record no call


# ---------------------------------------------------------------- ABI
def test_new_symbols_are_declared_bound_and_exported():
    from ign_hip import _lib
    assert _header_params(MIX) == ["x_btc", "out_btc", "len_b", "lam_b", "span_b2", "roll", "B", "T", "C", "stream"]
    assert _header_params(LOSS) == ["sbm", "dnn", "labels", "labels_b", "lam_b", "class_w", "reg", "out", "eta", "loss3", "gsbm", "gdnn",
                                    "B", "N", "beta", "label_smoothing", "stream"]
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.SIGNATURES[MIX] == (ci, [vp] * 5 + [ci] * 4 + [vp])
    assert _lib.SIGNATURES[LOSS] == (ci, [vp] * 12 + [ci, ci, cf, cf, vp])
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    h = ctypes.CDLL(_lib.lib_path())
    assert hasattr(h, MIX) and hasattr(h, LOSS)


def test_entry_points_refuse_bad_arguments_without_a_device():
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    h = _lib.lib()
    E_ARG, E_UNSUP, E_TOOBIG = -1001, -1002, -1003
    p, q, r = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24), ctypes.c_void_p(64)

    def mix(x=p, out=q, lam=r, roll=1, B=2, T=8, C=3):
        return h.ign_mix_btc(x, out, None, lam, None, roll, B, T, C, None)
    assert mix(out=p) == E_ARG and b"overlap" in h.ign_last_error()
    assert mix(out=ctypes.c_void_p((1 << 20) + 4 * (2 * 8 * 3 - 1))) == E_ARG                 # the last element of x
    assert mix(x=ctypes.c_void_p((1 << 24) + 4)) == E_ARG                                     # x begins inside out
    for kw in (dict(roll=2), dict(roll=-1), dict(T=0), dict(B=0), dict(C=0), dict(x=None), dict(out=None), dict(lam=None),
               dict(B=1, roll=1)):
        assert mix(**kw) == E_ARG, kw
    assert b"ign_mix_btc" in h.ign_last_error()
    assert mix(T=1 << 20, C=1 << 11, out=ctypes.c_void_p(1 << 60)) == E_TOOBIG

    def loss(B=4, N=3, eps=0.1, ya=r, yb=r, lam=r):
        return h.ign_loss_mix_fwd_bwd_reg(r, r, ya, yb, lam, None, None, r, r, r, r, r, B, N, 0.5, eps, None)
    for kw in (dict(B=0), dict(N=1), dict(eps=1.0), dict(eps=-0.1), dict(eps=float("nan")), dict(ya=None), dict(yb=None),
               dict(lam=None)):
        assert loss(**kw) == E_ARG, kw
    assert b"ign_loss_mix_fwd_bwd_reg" in h.ign_last_error()
    assert loss(N=257) == E_UNSUP
