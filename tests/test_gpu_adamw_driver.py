"""The harness with --weight_decay / --lr_schedule / --ema on the GPU (SYNTH provider at the BasicMotions shape: C 6, T 100, batch 8,
two epochs of three steps): default flags make none of the new calls and repeat the run of a namespace without them; with the
flags on, --hipgraph equals the eager run to the bit from ONE captured closing step, also with accumulation and clipping; the
checkpoint holds the averaged weights; validation hands the live weights back untouched; the average respects --pos_weight; SBM and
the regression task run with all three; the refused combinations raise before anything is built."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NEW = ("ign_adamw_step_dev", "ign_ema_update", "ign_swap_flat")
ON = ("--weight_decay", "0.01", "--lr_schedule", "cosine,warmup=2", "--ema", "0.9")
ACC = ("--gradient_accumulation_steps", "2", "--gradient_clip", "0.5")
FLAGS = ("weight_decay", "lr_schedule", "ema")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import speech_imagery_eeg_amd  # noqa: F401
    return torch.device("cuda:0")


def _experiment(tag, extra=(), drop_flags=False, model="InterpGN"):
    import run
    from exp.experiment_classification import Experiment
    argv = ["--model", model, "--dnn_type", "FCN", "--data", "SYNTH", "--synthetic", "24,6,100,4", "--dataset", "adamw" + tag,
            "--batch_size", "8", "--train_epochs", "2", "--num_workers", "0", "--seed", "0", "--patience", "10", "--amp"] + list(extra)
    a = run.get_args(argv)                                   # sic: --amp turns the bf16 autocast OFF
    if drop_flags:
        for k in FLAGS:
            delattr(a, k)                                    # the namespace of a caller that predates the flags
    run.set_seed(0)
    return Experiment(a)


def _train(e):
    torch.manual_seed(123)
    losses, step = [], 0
    for epoch in range(2):
        ls, step = e.train_one_epoch(epoch, step)
        losses += [float(l) for l in ls]
    ema = None if e.optimizer.ema_flat is None else e.optimizer.ema_flat.cpu().clone()
    return losses, {k: v.detach().float().cpu().clone() for k, v in e.model.state_dict().items()}, ema


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """tag -> (losses, final state, final EMA buffer, entry points called, {kind: captures}); each configuration trained once"""
    _dev()
    from ign_hip import _lib, graph
    L = _lib.lib()
    cwd = os.getcwd()
    os.chdir(tmp_path_factory.mktemp("adamw"))
    real = {k: getattr(L, k) for k in NEW}
    real_graphed = graph.GraphedTrainStep
    called, captures, off = [], {}, []

    def counted(name):
        def fn(*a):
            if off:
                raise AssertionError(f"{name} called with the flags at their defaults")
            called.append(name)
            return real[name](*a)
        return fn

    class Counted(real_graphed):
        def __init__(self, step_fn, example_inputs, warmup=3):
            kind = "micro" if step_fn.__name__ == "micro_fn" else "close"
            captures[kind] = captures.get(kind, 0) + 1
            super().__init__(step_fn, example_inputs, warmup=warmup)

    out = {}
    try:
        for k in NEW:
            setattr(L, k, counted(k))
        graph.GraphedTrainStep = Counted
        for tag, extra, drop in (("absent", (), True), ("default", (), False), ("eager", ON, False), ("graph", ON + ("--hipgraph",), False),
                                 ("acc_eager", ON + ACC, False), ("acc_graph", ON + ACC + ("--hipgraph",), False)):
            del called[:]
            captures.clear()
            off[:] = [tag] if tag in ("absent", "default") else []        # those two runs: every new entry point raises
            e = _experiment(tag, extra, drop)
            assert e._optim_active == (tag not in ("absent", "default")) and e.optimizer.scheduled == e._optim_active
            out[tag] = _train(e) + (list(called), dict(captures))
            if "graph" in tag:
                assert getattr(e, "_graphed", None) is not None and e._graph_eligible(False)       # the graph path really ran
            if tag == "acc_eager":
                assert e.optimizer.total_steps == 3 and int(e.optimizer.step_dev) == 3
            if tag == "eager":
                assert e.optimizer.total_steps == 6 and int(e.optimizer.step_dev) == 6
                # the record the last tick left: the cosine's end (the floor, 0) and the warmed-up decay min(0.9, 7/16)
                hp = e.optimizer.hp_dev.cpu().numpy()
                assert abs(float(hp[2]) - e.optimizer.lr_at(6)) <= 1e-9 and float(hp[3]) == float(np.float32(7 / 16))
    finally:
        for k in NEW:
            setattr(L, k, real[k])
        graph.GraphedTrainStep = real_graphed
        os.chdir(cwd)
    return out


def test_default_flags_make_none_of_the_new_calls_and_repeat_the_run_without_them(runs):
    absent, default = runs["absent"], runs["default"]
    assert absent[3] == [] and default[3] == [] and absent[2] is None and default[2] is None
    assert len(default[0]) == 6 and all(np.isfinite(default[0])) and default[0] == absent[0]
    for k, v in default[1].items():
        assert torch.equal(v, absent[1][k]), k


def test_flags_on_change_the_run_and_call_one_adamw_and_one_ema_launch_per_step(runs):
    on, off = runs["eager"], runs["default"]
    assert on[3] == ["ign_adamw_step_dev", "ign_ema_update"] * 6
    assert all(np.isfinite(on[0])) and on[0][0] == off[0][0] and on[0] != off[0]
    assert runs["acc_eager"][3] == ["ign_adamw_step_dev", "ign_ema_update"] * 3          # closing steps only
    assert any(not torch.equal(v, off[1][k]) for k, v in on[1].items())
    assert not torch.equal(on[2], runs["acc_eager"][2])


@pytest.mark.parametrize("eager,graph", [("eager", "graph"), ("acc_eager", "acc_graph")], ids=["plain", "accumulate+clip"])
def test_hipgraph_equals_the_eager_run_from_one_capture(runs, eager, graph):
    a, b = runs[eager], runs[graph]
    for k, v in a[1].items():
        assert torch.equal(v, b[1][k]), k
    assert torch.equal(a[2], b[2])                                  # the EMA buffer
    assert len(a[0]) == len(b[0]) == 6 and all(abs(x - y) <= 1e-5 * max(1.0, abs(x)) for x, y in zip(a[0], b[0]))
    # the learning rate is read on the device: one closing capture (and one micro capture) serves both epochs
    assert b[4] == ({"close": 1} if eager == "eager" else {"close": 1, "micro": 1})
    assert 0 < len(b[3]) < len(a[3])                                # the replays do not pass the host


def _flat(e, state):
    """the trainable parameters of a state dict in the bucket's layout (the padding between the slots stays zero)"""
    out = torch.zeros_like(e.optimizer.flat_param)
    for (k, p), off in zip(((k, p) for k, p in e.model.named_parameters() if p.requires_grad), e.bucket.offsets):
        out[off:off + p.numel()] = state[k].reshape(-1).to(out.device)
    return out


def test_checkpoint_holds_the_averaged_weights_and_validation_returns_the_live_ones(tmp_path, monkeypatch):
    _dev()
    monkeypatch.chdir(tmp_path)
    e = _experiment("ckpt", ON + ("--pos_weight",))
    opt = e.optimizer
    head = e.model.sbm.output_layer.weight
    assert bool((head < 0).any())                                   # the clamp has work to do ...
    with e._averaged_weights():
        assert bool((head >= 0).all())                              # ... and the average starts inside the constraint
    emas, lives = [], []
    orig = e.train_one_epoch

    def rec(epoch, train_step=0):
        if lives:                                                   # validation and the checkpoint of the last epoch are over:
            assert torch.equal(opt.flat_param, lives[-1]) and torch.equal(opt.ema_flat, emas[-1])   # both back, to the bit
        out = orig(epoch, train_step)
        emas.append(opt.ema_flat.clone())                           # the hand-kept copies: what the epoch's validation must see
        lives.append(opt.flat_param.clone())
        return out
    monkeypatch.setattr(e, "train_one_epoch", rec)
    seen = []
    orig_val = e._val_metrics

    def val():
        seen.append(opt.flat_param.clone())
        return orig_val()
    monkeypatch.setattr(e, "_val_metrics", val)
    torch.manual_seed(123)
    e.train()
    assert len(emas) == len(seen) == 2
    for ema, live, s in zip(emas, lives, seen):
        assert torch.equal(s, ema) and not torch.equal(ema, live)   # validation ran on the average ...
    ck = torch.load(os.path.join(e.checkpoint_dir, "checkpoint.pth"), map_location="cpu", weights_only=True)
    assert list(ck) == list(e.model.state_dict())
    flat = _flat(e, ck)
    match = [i for i, ema in enumerate(emas) if torch.equal(flat, ema)]
    assert len(match) == 1 and all(not torch.equal(flat, live) for live in lives)       # ... and the checkpoint holds it
    assert torch.equal(opt.flat_param, emas[match[0]])              # train() reloads the best checkpoint
    # the averaged head weights of a --pos_weight run are non-negative, like the live ones
    off = dict(zip((k for k, p in e.model.named_parameters() if p.requires_grad), e.bucket.offsets))["sbm.output_layer.weight"]
    for ema, live in zip(emas, lives):
        assert bool((ema[off:off + head.numel()] >= 0).all()) and bool((live[off:off + head.numel()] >= 0).all())


def test_sbm_runs_with_all_three_flags_and_validation_leaves_the_live_weights_alone(tmp_path, monkeypatch):
    _dev()
    monkeypatch.chdir(tmp_path)
    e = _experiment("sbm", ON, model="SBM")
    opt = e.optimizer
    before = opt.flat_param.clone()
    losses, _ = e.train_one_epoch(0, 0)
    assert len(losses) == 3 and all(np.isfinite([float(l) for l in losses])) and int(opt.step_dev) == 3
    assert not torch.equal(opt.flat_param, before) and not torch.equal(opt.ema_flat, before)
    # the shapelet banks take no decay: their mask chunks are zero, the output layer's are one
    names = [k for k, p in e.model.named_parameters() if p.requires_grad]
    assert "output_layer.weight" in names and any(k.endswith(".weights") for k in names)
    mask = opt.decay_mask.cpu()
    for k, p, off in zip(names, e.bucket.params, e.bucket.offsets):
        chunks = mask[off // 64:(off + p.numel() + 63) // 64]
        if k == "output_layer.weight":
            assert bool(chunks.all()), k
        if k.endswith(".weights") or p.ndim < 2:
            assert not bool(chunks.any()), k
    # a validation pass on the averaged weights leaves the live weights and the average as they were, to the bit
    live, ema = opt.flat_param.clone(), opt.ema_flat.clone()
    assert not torch.equal(live, ema)
    plain = e.validation()
    with e._averaged_weights():
        assert torch.equal(opt.flat_param, ema) and torch.equal(opt.ema_flat, live)
        averaged = e.validation()
    assert torch.equal(opt.flat_param, live) and torch.equal(opt.ema_flat, ema)
    assert e.validation() == plain and np.isfinite(averaged[0])


def test_regression_runs_with_all_three_flags(tmp_path, monkeypatch):
    _dev()
    import run
    from data_provider.ts_reader import write_ts
    from exp.experiment_regression import Experiment
    d = tmp_path / "Burst"
    d.mkdir()
    for split, n, seed in (("TRAIN", 24, 1), ("TEST", 8, 2)):
        rng = np.random.RandomState(seed)
        amp = rng.rand(n) * 5
        write_ts(str(d / f"Burst_{split}.ts"), [rng.randn(3, 120) * 0.3 + a for a in amp], amp, regression=True)
    monkeypatch.chdir(tmp_path)
    a = run.get_args(["--task_name", "regression", "--data", "Monash", "--model", "InterpGN", "--dnn_type", "FCN", "--data_root",
                      str(tmp_path), "--dataset", "Burst", "--train_epochs", "1", "--batch_size", "8", "--seed", "0", "--amp",
                      "--num_shapelet", "2", "--lr", "5e-3"] + list(ON))
    run.set_seed(0)
    e = Experiment(a)
    assert e.optimizer.scheduled and e.optimizer.total_steps == 3
    e.train()
    assert int(e.optimizer.step_dev) == 3
    ck = torch.load(os.path.join(e.checkpoint_dir, "checkpoint.pth"), map_location="cpu", weights_only=True)
    # one epoch: the checkpoint is that epoch's average, which the optimizer still holds beside the reloaded weights
    assert torch.equal(_flat(e, ck), e.optimizer.ema_flat) and bool(torch.isfinite(e.optimizer.ema_flat).all())


@pytest.mark.parametrize("change,match", [(dict(lr_decay=True), "lr_decay"), (dict(shapelet_project=2), "shapelet_project"),
                                          (dict(weight_decay=-0.1), "weight_decay"), (dict(ema=1.0), "ema"),
                                          (dict(lr_schedule="cosine,warmup=-1"), "warmup"), (dict(lr_schedule="cosine,min=-1"), "min"),
                                          (dict(lr_schedule="cosine,min=1"), "above")])
def test_refused_combinations_raise_before_anything_is_built(tmp_path, monkeypatch, change, match):
    _dev()
    import run
    from exp.experiment_classification import Experiment
    monkeypatch.chdir(tmp_path)

    def refuse(self):
        raise AssertionError("nothing may be built")
    monkeypatch.setattr(Experiment, "_load_data", refuse)
    a = run.get_args(["--data", "SYNTH", "--synthetic", "24,6,100,4"] + list(ON))
    for k, v in change.items():
        setattr(a, k, v)
    with pytest.raises(ValueError, match=match):
        Experiment(a)
    assert not os.path.exists(tmp_path / "checkpoints")
