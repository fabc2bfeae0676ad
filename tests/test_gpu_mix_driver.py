"""The harness with --mix on the GPU (SYNTH provider, two epochs, a small shape with a ragged last batch, as the harness tests of
tests/test_gpu_augment.py): a mixed run is finite, differs from the plain run and repeats; `--mix none` is the run without the flag;
--hipgraph agrees with eager; --augment and a ragged batch go with it and evaluation never mixes; the torch composition serves SBM
and the bf16-autocast mode; the regression task refuses the flag."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
MIX = "mixup=0.4,cutmix=1"


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import speech_imagery_eeg_amd  # noqa: F401
    return torch.device("cuda:0")


def _experiment(tag, extra=(), drop_flag=False, model="InterpGN", fp32=True):
    import run
    from exp.experiment_classification import Experiment
    # 72 training samples in batches of 16: four full batches and a ragged one of 8
    argv = ["--model", model, "--dnn_type", "FCN", "--data", "SYNTH", "--synthetic", "72,4,48,3", "--dataset", "mix" + tag,
            "--batch_size", "16", "--train_epochs", "2", "--num_workers", "0", "--seed", "0", "--patience", "10"] \
        + (["--amp"] if fp32 else []) + list(extra)                 # sic: --amp turns the bf16 autocast OFF
    a = run.get_args(argv)
    if drop_flag:
        del a.mix                                            # the namespace of a caller that predates the flag
    run.set_seed(0)
    return Experiment(a)


def _train(e):
    torch.manual_seed(123)
    losses, step = [], 0
    for epoch in range(2):
        ls, step = e.train_one_epoch(epoch, step)
        losses += [float(l) for l in ls]
    return losses, {k: v.detach().float().cpu().clone() for k, v in e.model.state_dict().items()}, e.validation()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the trainings the harness tests share: off (flag absent / none), on (twice), on under --hipgraph; with the number of
    ops.mix launches and of soft-label loss calls of each"""
    _dev()
    from ign_hip import ops
    cwd = os.getcwd()
    os.chdir(tmp_path_factory.mktemp("mix"))
    try:
        out, calls, soft = {}, [], []
        real_mix, real_loss = ops.mix, ops.ign_loss

        def counted(*a, **k):
            calls.append(1)
            return real_mix(*a, **k)

        def counted_loss(*a, **k):
            if k.get("lam") is not None:
                soft.append(1)
            return real_loss(*a, **k)
        ops.mix, ops.ign_loss = counted, counted_loss
        try:
            for tag, extra, drop in (("absent", (), True), ("none", ("--mix", "none"), False), ("on", ("--mix", MIX), False),
                                     ("again", ("--mix", MIX), False), ("graph", ("--mix", MIX, "--hipgraph"), False)):
                del calls[:], soft[:]
                e = _experiment(tag, extra, drop)
                assert (e._transforms.mix is None) == (tag in ("absent", "none"))
                out[tag] = _train(e) + (len(calls), len(soft))
                if tag == "graph":
                    assert getattr(e, "_graphed", None) is not None and e.optimizer.capturable     # the graph path really ran
        finally:
            ops.mix, ops.ign_loss = real_mix, real_loss
        return out
    finally:
        os.chdir(cwd)


def test_mixed_run_is_finite_different_and_repeatable(runs):
    on, again, off = runs["on"], runs["again"], runs["none"]
    assert len(on[0]) == len(off[0]) == 10 and all(np.isfinite(on[0]))
    assert on[3] == on[4] == len(on[0]) and off[3] == off[4] == 0     # one mix launch and one soft-label tail per step; none when off
    assert on[0] != off[0]
    assert on[0] == again[0] and on[2] == again[2]
    for k, v in on[1].items():
        assert torch.equal(v, again[1][k]), k


def test_none_is_the_run_without_the_flag(runs):
    assert runs["none"][0] == runs["absent"][0] and runs["none"][2] == runs["absent"][2] and runs["absent"][3] == 0
    for k, v in runs["none"][1].items():
        assert torch.equal(v, runs["absent"][1][k]), k


def test_hipgraph_agrees_with_eager(runs):
    """the criterion of test_gpu_driver.py::test_hipgraph_harness_run_equals_the_eager_run: validation numbers and final weights
    within 1e-5 of max(1, |value|); the per-step losses too"""
    eager, graph = runs["on"], runs["graph"]
    assert graph[3] == len(graph[0]) == len(eager[0])                 # mixed outside the capture: one launch per step, replayed or not
    assert 0 < graph[4] < eager[4]                                    # the soft-label tail was captured: replays do not pass the host
    for la, lb in zip(eager[0], graph[0]):
        assert abs(la - lb) <= 1e-5 * max(1.0, abs(la))
    (vl_a, va_a), (vl_b, va_b) = eager[2], graph[2]
    assert abs(vl_a - vl_b) <= 1e-5 * max(1.0, abs(vl_a)) and va_a == va_b
    for k, v in eager[1].items():
        w = graph[1][k]
        assert float((v - w).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max())), k


def test_with_augment_and_a_ragged_batch_and_evaluation_untouched(tmp_path, monkeypatch):
    dev = _dev()
    from ign_hip import ops
    from utils.augment import step_seed
    from utils.mix import mix_draws
    monkeypatch.chdir(tmp_path)
    e, plain = _experiment("rag", ("--mix", MIX, "--augment", "shift=0.1")), _experiment("rag0")
    # _mix on a ragged batch: the draws are mix_draws' under the step seed, every sample is mixed inside its own length
    B, T, C = 6, 48, 4
    lens = [48, 1, 0, 17, 30, 5]
    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(5)).to(dev)
    label = torch.arange(B, device=dev) % 3
    mask = torch.zeros(B, T, device=dev)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
        x[b, n:] = 777.0
    import dataclasses
    only_mix = dataclasses.replace(e._transforms, augment=None)      # the chain's mix stage on its own: same spec, base seed and rank
    out, (label_b, lam) = only_mix(x, label, mask, 3)
    roll, lam_h, span_h = mix_draws(step_seed(0, 0, 3), B, np.asarray(lens), e._transforms.mix)
    assert torch.equal(lam.cpu(), torch.from_numpy(lam_h)) and torch.equal(label_b, label[(torch.arange(B, device=dev) + roll) % B])
    want = ops.mix(x, lam, roll, span=torch.from_numpy(span_h).to(dev), lengths=torch.tensor(lens, dtype=torch.int32, device=dev))
    assert torch.equal(out, want)
    for b, n in enumerate(lens):
        assert bool((out[b, n:] == 777.0).all())
    assert plain._transforms.mix is None and plain._transforms(x, label, mask, 3) == (x, ())
    # validation() and test() never mix: same weights (same seed), same numbers, no launch
    for (n1, p1), (n2, p2) in zip(e.model.state_dict().items(), plain.model.state_dict().items()):
        assert n1 == n2 and torch.equal(p1, p2)

    def refuse(*a, **k):
        raise AssertionError("evaluation must not mix")
    real = ops.mix
    monkeypatch.setattr(ops, "mix", refuse)
    assert e.validation() == plain.validation()
    (l1, r1, _), (l2, r2, _) = e.test(save_csv=False), plain.test(save_csv=False)
    assert l1 == l2 and torch.equal(r1.preds, r2.preds) and torch.equal(r1.x_data, r2.x_data)
    monkeypatch.setattr(ops, "mix", real)
    # and the training loop runs with both flags over the ragged last batch
    losses, _, _ = _train(e)
    assert len(losses) == 10 and all(np.isfinite(losses))


@pytest.mark.parametrize("model,fp32", [("SBM", True), ("SBM", False), ("InterpGN", False)], ids=["SBM-fp32", "SBM-bf16", "InterpGN-bf16"])
def test_torch_composition_serves_sbm_and_bf16_autocast(tmp_path, monkeypatch, model, fp32):
    _dev()
    from ign_hip import ops
    from utils import mix as M
    monkeypatch.chdir(tmp_path)
    calls = []
    real = M.mix_cross_entropy

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(M, "mix_cross_entropy", counted)

    def refuse(*a, **k):
        raise AssertionError("the fused tail is InterpGN's fp32 route")
    monkeypatch.setattr(ops, "ign_loss", refuse)
    losses, _, _ = _train(_experiment("tc" + model, ("--mix", MIX), model=model, fp32=fp32))
    assert len(losses) == 10 and all(np.isfinite(losses))
    assert len(calls) == len(losses) * (2 if model == "InterpGN" else 1)


def test_regression_refuses_the_flag():
    _dev()
    import run
    from exp.experiment_regression import Experiment
    with pytest.raises(ValueError, match="regression"):
        run.get_args(["--data", "SYNTH", "--task_name", "regression", "--mix", "mixup=0.4"])
    e = Experiment.__new__(Experiment)                       # the set-up step itself, for a caller that builds its own namespace
    e.args, e.rank = Namespace(mix="mixup=0.4", task_name="regression", seed=0), 0
    with pytest.raises(ValueError, match="regression"):
        e._resolve_train_transforms()
    e.args = Namespace(mix="none", task_name="regression", seed=0)
    e._resolve_train_transforms()
    assert e._transforms.mix is None
