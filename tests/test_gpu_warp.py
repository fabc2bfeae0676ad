"""ops.warp / ign_warp_btc on the GPU against the numpy restatement of the rule (utils/warp.py:warp_reference), bit for bit on every
case of tests/warp_cases.py; padding and unwarped samples byte-identical to the input; a pre-filled output fully overwritten;
repeatability; a sample's result independent of the batch around it and of the buffers' alignment; the refusals (nothing launched);
the launch counter; and the harness with --warp (eager against --hipgraph, `none` against the run without the flag).

NaN compares equal to NaN (warp_cases.same_bits): the sign and payload of a NaN that inf - inf produces is the processor's
convention, not the rule's.  Every other value is compared by its 32 bits."""
import ctypes
import os

import numpy as np
import pytest
import torch

from warp_cases import ALL, CASES, IDS, SEED, SENTINEL, make_input, nonfinite_input, same_bits

pytestmark = pytest.mark.gpu
FILL = -12345.0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import speech_imagery_eeg_amd  # noqa: F401
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ref():
    """numpy restatements, computed once per case and left unchanged"""
    import speech_imagery_eeg_amd  # noqa: F401
    from utils.warp import warp_reference
    memo = {}

    def get(case):
        if case.id not in memo:
            x, lens = make_input(case)
            want = warp_reference(x, case.seed, lens, **case.kw)
            for a in (x, want):
                a.setflags(write=False)
            memo[case.id] = (x, lens, want)
        return memo[case.id]
    return get


def _raw(x, out, lens, seed, twarp=0.0, mwarp=0.0, wwarp=0.0, knots=4, prob=1.0):
    from ign_hip import _lib
    B, T, C = x.shape
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    return _lib.lib().ign_warp_btc(p(x), p(out), p(lens), B, T, C, seed, twarp, mwarp, wwarp, knots, prob, _lib.stream())


# ---------------------------------------------------------------- 1. bitwise, every case
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bitwise_equal_to_the_numpy_restatement(ref, case):
    dev = _dev()
    from ign_hip import ops
    x, lens, want = ref(case)
    xd = torch.from_numpy(x.copy()).to(dev)
    ld = None if lens is None else torch.from_numpy(lens).to(dev)
    out = ops.warp(xd, case.seed, lengths=ld, **case.kw)
    assert out.data_ptr() != xd.data_ptr() and np.array_equal(xd.cpu().numpy(), x), "the input is left as it was"
    got = out.cpu().numpy()
    assert got.dtype == want.dtype and same_bits(got, want)
    # the entry point itself, into an output that held something else: every element is written; and a second call gives the same bits
    pre = torch.full_like(xd, FILL)
    assert _raw(xd, pre, ld, case.seed, **case.kw) == 0
    again = pre.cpu().numpy()
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    # padding, and samples the rule leaves alone, are the input's bytes
    from utils.warp import sample_draws
    for b in range(case.B):
        n = case.T if lens is None else int(lens[b])
        assert np.array_equal(got[b, n:].view(np.uint32), x[b, n:].view(np.uint32))
        if lens is not None:
            assert (got[b, n:] == SENTINEL).all()
        if n < 2 or not sample_draws(case.seed, b, n, case.kw.get("wwarp", 0.0), case.kw.get("prob", 1.0))[0]:
            assert np.array_equal(got[b].view(np.uint32), x[b].view(np.uint32)), b
    if case.T >= 63:
        assert not np.array_equal(got, x)                    # the case exercises something
    if "prob" in case.kw:
        same = [np.array_equal(got[b], x[b]) for b in range(case.B)]
        assert any(same) and not all(same)                   # both kinds of sample occur


def test_all_rates_zero_is_a_copy_in_one_launch():
    dev = _dev()
    from ign_hip import _lib, ops
    x = torch.randn(3, 17, 5, device=dev)
    x[1, 4] = float("nan")
    _lib.timing_enable(True)
    try:
        out = ops.warp(x, SEED, knots=7, prob=0.5)
        torch.cuda.synchronize()
        assert _lib.timing_read("warp")[1] == 1
    finally:
        _lib.timing_enable(False)
    assert out.data_ptr() != x.data_ptr() and np.array_equal(out.cpu().numpy().view(np.uint32), x.cpu().numpy().view(np.uint32))


def test_nonfinite_neighbours_do_not_leak_through_weight_zero():
    dev = _dev()
    from ign_hip import ops
    from utils.warp import warp_reference
    x = nonfinite_input()
    for kw in (dict(twarp=0.3), dict(ALL)):
        got = ops.warp(torch.from_numpy(x).to(dev), SEED, **kw).cpu().numpy()
        assert same_bits(got, warp_reference(x, SEED, **kw))
        assert np.isfinite(got[0, 0]).all() and np.isfinite(got[1, 0, [0, 1, 3]]).all() and got[1, 0, 2] == -np.inf
        if "mwarp" not in kw:
            assert np.array_equal(got[:, 0].view(np.uint32), x[:, 0].view(np.uint32))       # phi(0) = 0: a copy


# ---------------------------------------------------------------- 2. purity
@pytest.mark.parametrize("cid", ["5x64x122-ragged", "5x65x3-knots1"])
def test_a_sample_does_not_depend_on_the_batch_around_it(ref, cid):
    dev = _dev()
    from ign_hip import ops
    case = next(c for c in CASES if c.id == cid)
    x, lens, want = ref(case)
    xd = torch.from_numpy(x.copy()).to(dev)
    ld = None if lens is None else torch.from_numpy(lens).to(dev)
    for b in range(case.B):
        part = ops.warp(xd[:b + 1].contiguous(), case.seed, lengths=None if ld is None else ld[:b + 1].contiguous(), **case.kw)
        assert np.array_equal(part[b].cpu().numpy().view(np.uint32), want[b].view(np.uint32)), b


@pytest.mark.parametrize("cid", ["1x64x4-knots8", "5x64x122-ragged"])
def test_buffers_that_are_only_4_byte_aligned(ref, cid):
    """the 16- and 8-byte paths need aligned buffers; a batch that starts one float into its allocation takes the single-float path
    and gives the same bits"""
    dev = _dev()
    from ign_hip import ops
    case = next(c for c in CASES if c.id == cid)
    x, lens, want = ref(case)
    flat = torch.empty(x.size + 1, device=dev)
    xd = flat[1:].view(x.shape)
    xd.copy_(torch.from_numpy(x.copy()))
    assert xd.data_ptr() % 8 == 4 and xd.is_contiguous()
    ld = None if lens is None else torch.from_numpy(lens).to(dev)
    got = ops.warp(xd, case.seed, lengths=ld, **case.kw).cpu().numpy()
    assert same_bits(got, want)
    oflat = torch.full((x.size + 1,), FILL, device=dev)
    od = oflat[1:].view(x.shape)
    aligned = torch.from_numpy(x.copy()).to(dev)
    assert _raw(aligned, od, ld, case.seed, **case.kw) == 0
    assert same_bits(od.cpu().numpy(), want) and float(oflat[0]) == FILL


# ---------------------------------------------------------------- 3. refusals and the launch counter
def test_refusals_launch_nothing():
    dev = _dev()
    from ign_hip import _lib, ops
    L = _lib.lib()
    x = torch.randn(2, 8, 3, device=dev)
    keep = x.clone()
    out = torch.full_like(x, 5.0)
    _lib.timing_enable(True)
    try:
        assert _raw(x, x, None, 7, twarp=0.1) == -1001                                      # IGN_E_ARG
        msg = L.ign_last_error().decode()
        assert "ign_warp_btc" in msg and "overlap" in msg
        both = torch.zeros(2 * x.numel() - 3, device=dev)                                   # out begins inside x's last row
        assert _raw(both[:x.numel()].view(x.shape), both[x.numel() - 3:].view(x.shape), None, 7, twarp=0.1) == -1001
        for kw in (dict(twarp=1.0), dict(mwarp=1.0), dict(wwarp=1.0), dict(twarp=float("nan")), dict(twarp=0.1, knots=0),
                   dict(twarp=0.1, knots=9), dict(twarp=0.1, prob=0.0), dict(twarp=0.1, prob=1.5)):
            assert _raw(x, out, None, 7, **kw) == -1001, kw
        assert _raw(x, None, None, 7, twarp=0.1) == -1001
        torch.cuda.synchronize()
        assert _lib.timing_read("warp")[1] == 0                                             # nothing was launched
        assert torch.equal(x, keep) and bool((out == 5.0).all())
        for n in (1, 2, 3):                                                                 # exactly one launch per call
            ops.warp(x, n, **ALL)
            torch.cuda.synchronize()
            assert _lib.timing_read("warp")[1] == n
    finally:
        _lib.timing_enable(False)
    with pytest.raises(_lib.IgnError):
        ops.warp(x.clone().requires_grad_(True), 1, twarp=0.1)
    with pytest.raises(_lib.IgnError):
        ops.warp(x.permute(0, 2, 1), 1, twarp=0.1)
    with pytest.raises(_lib.IgnError):
        ops.warp(x.double(), 1, twarp=0.1)
    with pytest.raises(_lib.IgnError):
        ops.warp(x.cpu(), 1, twarp=0.1)
    with pytest.raises(_lib.IgnError):
        ops.warp(x, 1, twarp=0.1, lengths=torch.tensor([8, 8], device=dev))                 # int64
    for kw in (dict(twarp=1.0), dict(mwarp=-0.25), dict(twarp=0.1, knots=9), dict(twarp=0.1, prob=0.0)):
        with pytest.raises(ValueError):
            ops.warp(x, 1, **kw)


def test_refused_during_capture():
    dev = _dev()
    from ign_hip import _lib, ops
    x = torch.randn(2, 8, 3, device=dev)
    ops.warp(x, 1, twarp=0.1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.IgnError, match="capture"):             # as ops.augment (test_gpu_augment.py)
        with torch.cuda.graph(g):
            ops.warp(x, 1, twarp=0.1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 4. the harness
WARP = "twarp=0.2,mwarp=0.1,wwarp=0.1"


def _experiment(tag, extra=(), drop_flag=False, task=()):
    import run
    from exp.experiment_classification import Experiment
    # 32 training samples in batches of 16: two training steps (under --hipgraph: one eager, one replayed)
    argv = ["--model", "InterpGN", "--dnn_type", "FCN", "--data", "SYNTH", "--synthetic", "32,4,48,3", "--dataset", "warp" + tag,
            "--batch_size", "16", "--amp", "--train_epochs", "1", "--num_workers", "0", "--seed", "0", "--patience", "10"] + list(extra)
    a = run.get_args(argv)
    if drop_flag:
        del a.warp                                           # the namespace of a caller that predates the flag
    run.set_seed(0)
    return Experiment(a)


def _train(e):
    torch.manual_seed(123)
    ls, _ = e.train_one_epoch(0, 0)
    return [float(l) for l in ls], {k: v.detach().float().cpu().clone() for k, v in e.model.state_dict().items()}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the trainings the harness tests share: off (flag absent / none, the latter with the launch counter on), on, on under
    --hipgraph; with the number of ops.warp calls of each"""
    _dev()
    from ign_hip import _lib, ops
    cwd = os.getcwd()
    os.chdir(tmp_path_factory.mktemp("warp"))
    try:
        out, calls = {}, []
        real = ops.warp

        def counted(*a, **k):
            calls.append(1)
            return real(*a, **k)
        ops.warp = counted
        try:
            for tag, extra, drop in (("absent", (), True), ("none", ("--warp", "none"), False), ("on", ("--warp", WARP), False),
                                     ("graph", ("--warp", WARP, "--hipgraph"), False)):
                del calls[:]
                e = _experiment(tag, extra, drop)
                assert (e._transforms.warp is None) == (tag in ("absent", "none"))
                launches = None
                if tag == "none":
                    _lib.timing_enable(True)
                try:
                    res = _train(e)
                    if tag == "none":
                        torch.cuda.synchronize()
                        launches = _lib.timing_read("warp")[1]
                finally:
                    if tag == "none":
                        _lib.timing_enable(False)
                out[tag] = res + (len(calls), launches)
                if tag == "graph":
                    assert getattr(e, "_graphed", None) is not None and e.optimizer.capturable     # the graph path really ran
        finally:
            ops.warp = real
        return out
    finally:
        os.chdir(cwd)


def test_harness_eager_and_hipgraph_losses_are_bitwise_equal(runs):
    eager, graph, off = runs["on"], runs["graph"], runs["none"]
    print("warp harness losses: eager", [l.hex() for l in eager[0]], "graph", [l.hex() for l in graph[0]], "off", off[0])
    assert len(eager[0]) == len(graph[0]) == len(off[0]) == 2 and all(np.isfinite(eager[0]))
    assert eager[2] == graph[2] == 2                         # warped outside the capture: one launch per step, replayed or not
    assert eager[0] != off[0]                                # the flag does something
    assert eager[0] == graph[0]                              # floats compared exactly: the same draws, the same batch, the same step


def test_harness_none_is_the_run_without_the_flag(runs):
    assert runs["none"][0] == runs["absent"][0]
    assert runs["none"][2] == runs["absent"][2] == 0 and runs["none"][3] == 0            # no call and no launch
    for k, v in runs["none"][1].items():
        assert torch.equal(v, runs["absent"][1][k]), k


def test_harness_ragged_batch_regression_and_evaluation_untouched(tmp_path, monkeypatch):
    dev = _dev()
    from ign_hip import ops
    from utils.augment import step_seed
    monkeypatch.chdir(tmp_path)
    e, plain = _experiment("rag", ("--warp", WARP)), _experiment("rag0")
    B, T, C = 6, 48, 4
    lens = [48, 1, 0, 17, 30, 5]
    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(5)).to(dev)
    mask = torch.zeros(B, T, device=dev)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
        x[b, n:] = SENTINEL
    out, soft = e._transforms(x, None, mask, 3)                   # --warp alone: the chain is that one stage
    assert soft == () and (e._transforms.augment, e._transforms.mix) == (None, None)
    for b, n in enumerate(lens):
        assert bool((out[b, n:] == SENTINEL).all())
        assert n < 3 or not torch.equal(out[b, :n], x[b, :n])
    spec = e._transforms.warp._asdict()
    want = ops.warp(x, step_seed(0, 0, 3), lengths=torch.tensor(lens, dtype=torch.int32, device=dev), **spec)
    assert torch.equal(out, want)
    assert torch.equal(e._transforms(x, None, torch.ones(B, T, device=dev), 3)[0], ops.warp(x, step_seed(0, 0, 3), **spec))
    assert plain._transforms.warp is None and plain._transforms(x, None, mask, 3)[0] is x
    # validation() and test() never warp: same weights (same seed), same numbers, no launch
    for (n1, p1), (n2, p2) in zip(e.model.state_dict().items(), plain.model.state_dict().items()):
        assert n1 == n2 and torch.equal(p1, p2)

    def refuse(*a, **k):
        raise AssertionError("evaluation must not warp")
    monkeypatch.setattr(ops, "warp", refuse)
    assert e.validation() == plain.validation()
    (l1, r1, _), (l2, r2, _) = e.test(save_csv=False), plain.test(save_csv=False)
    assert l1 == l2 and torch.equal(r1.preds, r2.preds) and torch.equal(r1.x_data, r2.x_data)
    monkeypatch.undo()
    monkeypatch.chdir(tmp_path)
    # --task_name regression takes the flag: one warp per training step, finite losses
    import run
    from exp.experiment_regression import Experiment as Regression
    from data_provider.ts_reader import write_ts
    os.makedirs(tmp_path / "Ramp")
    rng = np.random.RandomState(1)
    for split, n in (("TRAIN", 32), ("TEST", 16)):               # a Monash-format set: the target is the mean level of the trial
        level = rng.rand(n) * 5
        write_ts(str(tmp_path / "Ramp" / f"Ramp_{split}.ts"), [rng.randn(3, 48) * 0.3 + v for v in level], level, regression=True)
    a = run.get_args(["--task_name", "regression", "--data", "Monash", "--model", "InterpGN", "--dnn_type", "FCN", "--data_root",
                      str(tmp_path), "--dataset", "Ramp", "--train_epochs", "1", "--batch_size", "16", "--seed", "0", "--amp",
                      "--num_shapelet", "4", "--patience", "10", "--warp", WARP])
    run.set_seed(0)
    r = Regression(a)
    calls, real = [], ops.warp
    monkeypatch.setattr(ops, "warp", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    losses, _ = r.train_one_epoch(0, 0)
    assert len(calls) == len(losses) == 2 and all(np.isfinite([float(l) for l in losses]))
