"""ops.augment / ign_augment_btc on the GPU against the numpy restatement of the rule (utils/augment.py): bitwise without noise,
to a derived bound with noise, repeatability and purity, the refusals, and the harness with --augment (eager, --hipgraph, ragged,
off, and validation / test left alone).

Input: randn plus a per-channel offset in [-2, 2]; the padding of a ragged batch holds a sentinel, not zero.

Noise bound |out - ref64| <= 1e-5 * sigma + 2^-22 * |ref64|: the 24-bit uniforms are exact; logf, sqrtf and sincosf are within 4 ulp
each (OpenCL-grade); the fp32 rounding of 2 pi u2 moves the angle by at most 4e-7; |n| <= 5.77: under 6e-6 in n, so under 6e-6 * sigma
in the output; the roundings of a, a * x, sigma * n and the sum are each 2^-24 relative, covered by 2^-22 |ref| and, where the sum
cancels, by the slack of the first term (|a x| <= 12 here: 12 * 2^-23 = 1.4e-6 against 2e-6 of slack at sigma = 0.5)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SEED = 0x0123456789ABCDEF
SENTINEL = 777.0
# (1,2,1) smallest; (3,7,5) nothing aligned, partial tail quad; (2,64,4) everything aligned; (2,65,122) CHISCO's channel count, quads
# straddle rows; (5,33,3) ragged: full, length 1 (shift and span forced to 0), 2, 17, empty; (70,9,2) more samples than a wave has lanes
SHAPES = [(1, 2, 1, None), (3, 7, 5, None), (2, 64, 4, None), (2, 65, 122, None), (5, 33, 3, (33, 1, 2, 17, 0)), (70, 9, 2, None)]
IDS = ["1x2x1", "3x7x5", "2x64x4", "2x65x122", "5x33x3-ragged", "70x9x2"]
RATES = dict(shift=0.3, scale=0.4, channel_drop=0.3, time_mask=0.5)
SETS = {k: {k: v} for k, v in RATES.items()}
SETS["all"] = dict(RATES)
SIGMA = 0.5
_WORST = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import speech_imagery_eeg_amd  # noqa: F401
    return torch.device("cuda:0")


def _case(B, T, C, lens):
    g = torch.Generator().manual_seed(1000 * B + 10 * T + C)
    x = torch.randn(B, T, C, generator=g) + (4 * torch.rand(C, generator=g) - 2)
    if lens is not None:
        for b, n in enumerate(lens):
            x[b, n:] = SENTINEL
    return x.contiguous(), (None if lens is None else np.asarray(lens, dtype=np.int32))


@pytest.fixture(scope="module")
def ref():
    """numpy restatements, computed once per (shape, options, dtype)"""
    import speech_imagery_eeg_amd  # noqa: F401
    from utils.augment import augment_reference
    memo = {}

    def get(i, dtype, **kw):
        key = (i, np.dtype(dtype).name, tuple(sorted(kw.items())))
        if key not in memo:
            x, lens = _case(*SHAPES[i])
            memo[key] = augment_reference(x.numpy(), SEED, lens, dtype=dtype, **kw)
            memo[key].setflags(write=False)
        return memo[key]
    return get


def _run(dev, x, lens, seed=SEED, **kw):
    from ign_hip import ops
    xd = x.to(dev)
    ld = None if lens is None else torch.from_numpy(lens).to(dev)
    out = ops.augment(xd, seed, lengths=ld, **kw)
    assert out.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), x), "the input is left as it was"
    return out.cpu()


# ---------------------------------------------------------------- 1. bitwise without noise
@pytest.mark.parametrize("which", list(SETS))
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_bitwise_equal_to_the_float32_restatement(ref, i, which):
    dev = _dev()
    x, lens = _case(*SHAPES[i])
    out = _run(dev, x, lens, **SETS[which]).numpy()
    want = ref(i, np.float32, **SETS[which])
    assert out.dtype == want.dtype and np.array_equal(out.view(np.uint32), want.view(np.uint32))
    if lens is not None:
        for b, n in enumerate(lens):
            assert (out[b, n:] == SENTINEL).all()
    if x.numel() > 64:
        assert not np.array_equal(out, x.numpy())            # the case exercises something


# ---------------------------------------------------------------- 2. with noise, against float64
@pytest.mark.parametrize("which", ["noise", "all"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_noise_against_the_float64_restatement(ref, i, which):
    dev = _dev()
    x, lens = _case(*SHAPES[i])
    kw = dict(noise=SIGMA, **(RATES if which == "all" else {}))
    out = _run(dev, x, lens, **kw).double().numpy()
    want = ref(i, np.float64, **kw)
    err = np.abs(out - want)
    bound = 1e-5 * SIGMA + 2.0 ** -22 * np.abs(want)
    worst = float((err / bound).max())
    _WORST[f"{IDS[i]}/{which}"] = dict(max_abs_err=float(err.max()), max_err_over_bound=worst)
    print(f"augment noise {IDS[i]} {which}: max |err| {err.max():.3e}, worst err / bound {worst:.3f}")
    assert (err <= bound).all(), _WORST[f"{IDS[i]}/{which}"]
    if lens is not None:
        for b, n in enumerate(lens):
            assert (out[b, n:] == SENTINEL).all()            # padding receives no noise
    if which == "noise" and lens is None:
        assert (out != x.double().numpy()).mean() > 0.9


@pytest.fixture(scope="module", autouse=True)
def _write_worst():
    yield
    path = os.environ.get("IGN_AUGMENT_NOISE_RECORD")           # a file to keep the observed errors in (profiles/augment.json)
    if _WORST and path:
        with open(path, "w") as f:
            json.dump(dict(sigma=SIGMA, bound="1e-5 * sigma + 2^-22 * |ref|", cases=_WORST), f, indent=1, sort_keys=True)


# ---------------------------------------------------------------- 3. repeatability and purity
@pytest.mark.parametrize("i", [1, 3, 4], ids=[IDS[1], IDS[3], IDS[4]])
def test_repeatable_and_seed_sensitive(i):
    dev = _dev()
    x, lens = _case(*SHAPES[i])
    kw = dict(noise=SIGMA, **RATES)
    a, b = _run(dev, x, lens, **kw), _run(dev, x, lens, **kw)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for bit in (0, 31, 32, 63):
        assert not torch.equal(a, _run(dev, x, lens, seed=SEED ^ (1 << bit), **kw)), bit


def test_a_sub_batch_equals_the_rows_of_the_batch():
    dev = _dev()
    for i in (3, 4, 5):
        x, lens = _case(*SHAPES[i])
        kw = dict(noise=SIGMA, **RATES)
        full = _run(dev, x, lens, **kw)
        part = _run(dev, x[:2].contiguous(), None if lens is None else lens[:2], **kw)
        assert torch.equal(part.view(torch.int32), full[:2].view(torch.int32)), IDS[i]


def test_full_lengths_equal_no_lengths_and_zero_rates_are_the_identity():
    dev = _dev()
    for i in (1, 3, 5):
        B, T, C, _ = SHAPES[i]
        x, _ = _case(*SHAPES[i])
        kw = dict(noise=SIGMA, **RATES)
        a, b = _run(dev, x, None, **kw), _run(dev, x, np.full(B, T, dtype=np.int32), **kw)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), IDS[i]
    for i in range(len(SHAPES)):
        x, lens = _case(*SHAPES[i])
        out = _run(dev, x, lens)
        assert torch.equal(out.view(torch.int32), x.view(torch.int32)), IDS[i]


# ---------------------------------------------------------------- 4. refusals
def test_refusals():
    dev = _dev()
    from ign_hip import _lib, ops
    x = torch.randn(2, 8, 3, device=dev)
    with pytest.raises(_lib.IgnError, match="requires a gradient"):
        ops.augment(x.clone().requires_grad_(True), 1, shift=0.1)
    with pytest.raises(_lib.IgnError, match="contiguous"):
        ops.augment(x.permute(0, 2, 1), 1, shift=0.1)
    with pytest.raises(_lib.IgnError, match="float32"):
        ops.augment(x.double(), 1, shift=0.1)
    with pytest.raises(_lib.IgnError):
        ops.augment(x.cpu(), 1, shift=0.1)
    with pytest.raises(_lib.IgnError, match="lengths"):
        ops.augment(x, 1, shift=0.1, lengths=torch.tensor([8, 8], device=dev))           # int64
    for k in ("shift", "scale", "channel_drop", "time_mask"):
        with pytest.raises(ValueError, match=k):
            ops.augment(x, 1, **{k: 1.0})
        with pytest.raises(ValueError, match=k):
            ops.augment(x, 1, **{k: -0.25})
    with pytest.raises(ValueError, match="noise"):
        ops.augment(x, 1, noise=-1.0)
    with pytest.raises(ValueError, match="noise"):
        ops.augment(x, 1, noise=float("inf"))


def test_c_abi_refuses_in_place_and_bad_rates():
    dev = _dev()
    from ign_hip import _lib
    L = _lib.lib()
    x = torch.randn(2, 8, 3, device=dev)
    keep = x.clone()
    out = torch.full_like(x, 5.0)
    p, q = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr())

    def call(src, dst, B=2, T=8, C=3, shift=0.1, scale=0.0, sigma=0.0, thr=0, tm=0.0):
        return L.ign_augment_btc(src, dst, None, B, T, C, 7, shift, scale, sigma, thr, tm, _lib.stream())
    assert call(p, p) == -1001                                                          # IGN_E_ARG
    msg = L.ign_last_error().decode()
    assert "ign_augment_btc" in msg and "overlap" in msg
    assert call(p, ctypes.c_void_p(x.data_ptr() + 4 * (2 * 8 * 3 - 1))) == -1001           # out at the last element of x
    assert call(ctypes.c_void_p(out.data_ptr() + 4), q) == -1001                        # x begins inside out
    for kw in (dict(shift=1.0), dict(scale=1.0), dict(tm=1.0), dict(thr=65536), dict(sigma=-1.0), dict(sigma=float("nan")),
               dict(shift=float("nan")), dict(T=0), dict(B=0), dict(C=0)):
        assert call(p, q, **kw) == -1001, kw
    assert call(None, q) == -1001 and call(p, None) == -1001
    assert call(p, q, C=8193) == -1003                                                  # IGN_E_TOOBIG (nothing is read)
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and bool((out == 5.0).all())                            # nothing was launched


def test_refused_during_capture():
    dev = _dev()
    from ign_hip import _lib, ops
    x = torch.randn(2, 8, 3, device=dev)
    ops.augment(x, 1, shift=0.1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.IgnError, match="capture"):             # as ops.attention with p > 0 (test_gpu_attn_dropout.py)
        with torch.cuda.graph(g):
            ops.augment(x, 1, shift=0.1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. the harness
AUG = "shift=0.1,scale=0.1,noise=0.05,chan_drop=0.2,time_mask=0.1"


def _experiment(tag, extra=(), drop_flag=False):
    import run
    from exp.experiment_classification import Experiment
    argv = ["--model", "InterpGN", "--dnn_type", "FCN", "--data", "SYNTH", "--synthetic", "64,4,48,3", "--dataset", "aug" + tag,
            "--batch_size", "16", "--amp", "--train_epochs", "2", "--num_workers", "0", "--seed", "0", "--patience", "10"] + list(extra)
    a = run.get_args(argv)
    if drop_flag:
        del a.augment                                        # the namespace of a caller that predates the flag
    run.set_seed(0)
    return Experiment(a)


def _train(e):
    torch.manual_seed(123)
    losses, step = [], 0
    for epoch in range(2):
        ls, step = e.train_one_epoch(epoch, step)
        losses += [float(l) for l in ls]
    return losses, {k: v.detach().float().cpu().clone() for k, v in e.model.state_dict().items()}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the trainings the harness tests share: off (flag absent / none), on (twice), on under --hipgraph"""
    _dev()
    from ign_hip import ops
    cwd = os.getcwd()
    os.chdir(tmp_path_factory.mktemp("augment"))
    try:
        out, calls = {}, []
        real = ops.augment

        def counted(*a, **k):
            calls.append(1)
            return real(*a, **k)
        ops.augment = counted
        try:
            for tag, extra, drop in (("absent", (), True), ("none", ("--augment", "none"), False), ("on", ("--augment", AUG), False),
                                     ("again", ("--augment", AUG), False), ("graph", ("--augment", AUG, "--hipgraph"), False)):
                del calls[:]
                e = _experiment(tag, extra, drop)
                out[tag] = _train(e) + (len(calls),)
                if tag == "graph":
                    assert getattr(e, "_graphed", None) is not None and e.optimizer.capturable     # the graph path really ran
        finally:
            ops.augment = real
        return out
    finally:
        os.chdir(cwd)


def test_harness_augmented_run_is_finite_different_and_repeatable(runs):
    on, again, off = runs["on"], runs["again"], runs["none"]
    assert len(on[0]) == len(off[0]) > 2 and all(np.isfinite(on[0]))
    assert on[2] == len(on[0]) and off[2] == 0               # one launch per training step; none when off
    assert on[0] != off[0]
    assert on[0] == again[0]
    for k, v in on[1].items():
        assert torch.equal(v, again[1][k]), k


def test_harness_none_is_the_run_without_the_flag(runs):
    assert runs["none"][0] == runs["absent"][0] and runs["absent"][2] == 0
    for k, v in runs["none"][1].items():
        assert torch.equal(v, runs["absent"][1][k]), k


def test_harness_hipgraph_agrees_with_eager(runs):
    """the criterion of test_gpu_class_weight.py's captured-versus-eager harness test: 1e-5 of max(1, |value|)"""
    eager, graph = runs["on"], runs["graph"]
    assert graph[2] == len(graph[0]) == len(eager[0])
    for la, lb in zip(eager[0], graph[0]):
        assert abs(la - lb) <= 1e-5 * max(1.0, abs(la))
    for k, v in eager[1].items():
        w = graph[1][k]
        assert float((v - w).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max())), k


def test_harness_ragged_batch_and_evaluation_untouched(tmp_path, monkeypatch):
    dev = _dev()
    from ign_hip import ops
    from utils.augment import step_seed
    monkeypatch.chdir(tmp_path)
    e, plain = _experiment("rag", ("--augment", AUG)), _experiment("rag0")
    B, T, C = 6, 48, 4
    lens = [48, 1, 0, 17, 30, 5]
    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(5)).to(dev)
    mask = torch.zeros(B, T, device=dev)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
        x[b, n:] = SENTINEL
    out, soft = e._transforms(x, None, mask, 3)                   # --augment alone: the chain is that one stage
    assert soft == () and (e._transforms.warp, e._transforms.mix) == (None, None)
    for b, n in enumerate(lens):
        assert bool((out[b, n:] == SENTINEL).all())
        assert n < 2 or not torch.equal(out[b, :n], x[b, :n])
    spec = e._transforms.augment._asdict()
    want = ops.augment(x, step_seed(0, 0, 3), lengths=torch.tensor(lens, dtype=torch.int32, device=dev), **spec)
    assert torch.equal(out, want)
    assert torch.equal(e._transforms(x, None, torch.ones(B, T, device=dev), 3)[0], ops.augment(x, step_seed(0, 0, 3), **spec))
    assert plain._transforms.augment is None and plain._transforms(x, None, mask, 3)[0] is x
    # validation() and test() never augment: same weights (same seed), same numbers, no launch
    for (n1, p1), (n2, p2) in zip(e.model.state_dict().items(), plain.model.state_dict().items()):
        assert n1 == n2 and torch.equal(p1, p2)

    def refuse(*a, **k):
        raise AssertionError("evaluation must not augment")
    monkeypatch.setattr(ops, "augment", refuse)
    assert e.validation() == plain.validation()
    (l1, r1, _), (l2, r2, _) = e.test(save_csv=False), plain.test(save_csv=False)
    assert l1 == l2 and torch.equal(r1.preds, r2.preds) and torch.equal(r1.x_data, r2.x_data)
