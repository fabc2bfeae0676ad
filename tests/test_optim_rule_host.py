"""AdamW, the per-step learning-rate schedule and the EMA of the weights, host side: the flag parser and the refused combinations,
the numpy rule (utils/optim_rule.py) against torch's CosineAnnealingLR and torch.optim.AdamW in float64, which parameters decay,
which entry point FlatAdam calls with which arguments, and -- when libign_hip.so is built -- the C rule (ign_sched_lr) against the
numpy one, the exported symbols and the argument checks.  Needs no device."""
import ctypes
import math
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import make_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ign_sched_lr", "ign_adamw_step_dev", "ign_ema_update", "ign_swap_flat")
E_ARG = -1001
SYNTH = ["--data", "SYNTH", "--synthetic", "24,6,100,4"]
# (W, S): no warm-up and a run of one step; no warm-up; the warm-up ends at the last step; warm-up then cosine; warm-up longer than the run
CASES = ((0, 1), (0, 7), (3, 3), (3, 10), (5, 4))
BASE, FLOOR = 5e-3, 1e-4


def _rule():
    import speech_imagery_eeg_amd  # noqa: F401
    from utils import optim_rule
    return optim_rule


def _lib_or_skip():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so is not built")
    return _lib.lib()


# ---------------------------------------------------------------- parser and refused combinations
def test_parser_accepts_the_specs():
    R = _rule()
    for text in (None, "", "none", "None"):
        assert R.parse_lr_schedule(text) == R.LrSchedule() and not R.parse_lr_schedule(text).active
    assert R.parse_lr_schedule("constant") == R.LrSchedule("constant", 0, 0.0)
    assert R.parse_lr_schedule("constant,warmup=4") == R.LrSchedule("constant", 4, 0.0)
    assert R.parse_lr_schedule("cosine") == R.LrSchedule("cosine", 0, 0.0)
    assert R.parse_lr_schedule("cosine,min=1e-4,warmup=2") == R.LrSchedule("cosine", 2, 1e-4)
    assert R.parse_lr_schedule(" cosine , warmup=2 ") == R.LrSchedule("cosine", 2, 0.0)
    spec = R.parse_lr_schedule("cosine,warmup=2")
    assert R.parse_lr_schedule(spec) is spec and spec.active
    assert (R.LrSchedule().code, R.parse_lr_schedule("constant").code, spec.code) == (0, 0, 1)


@pytest.mark.parametrize("text", ["linear", "cosine,restarts=2", "constant,min=1e-4", "cosine,warmup", "cosine,warmup=-1",
                                  "cosine,warmup=1.5", "cosine,min=-1e-4", "cosine,min=nan", "cosine,min=x", "cosine,warmup=1,warmup=2",
                                  "warmup=3"])
def test_parser_refuses(text):
    with pytest.raises(ValueError, match="lr_schedule"):
        _rule().parse_lr_schedule(text)


@pytest.mark.parametrize("extra,match", [
    (["--lr_schedule", "cosine", "--lr_decay"], "lr_decay"),
    (["--lr_schedule", "constant,warmup=3", "--lr_decay"], "lr_decay"),
    (["--ema", "0.99", "--shapelet_project", "2"], "shapelet_project"),
    (["--weight_decay", "-0.01"], "weight_decay"),
    (["--ema", "1.0"], "ema"),
    (["--ema", "-0.1"], "ema"),
    (["--lr_schedule", "cosine,warmup=-2"], "warmup"),
    (["--lr_schedule", "cosine,min=-1"], "min"),
    (["--lr_schedule", "cosine,min=0.1", "--lr", "0.005"], "above --lr"),
])
def test_check_args_refuses(extra, match):
    import speech_imagery_eeg_amd  # noqa: F401
    import run
    with pytest.raises(ValueError, match=match):
        run.get_args(SYNTH + extra)


def test_check_args_accepts_what_is_neutral_or_fine():
    import speech_imagery_eeg_amd  # noqa: F401
    import run
    R = _rule()
    a = run.get_args(SYNTH + ["--lr_decay", "--shapelet_project", "2"])
    assert (a.weight_decay, a.lr_schedule, a.ema) == (0.0, "none", 0.0)
    assert R.check_optim_options(a, flat_path=False) == (0.0, R.LrSchedule(), 0.0)
    assert R.check_optim_options(Namespace(lr=5e-3), flat_path=False) == (0.0, R.LrSchedule(), 0.0)     # a namespace before the flags
    ok = Namespace(lr=5e-3, weight_decay=0.01, lr_schedule="cosine,warmup=2,min=0.005", ema=0.9, shapelet_project="end", lr_decay=False)
    assert R.check_optim_options(ok, flat_path=True) == (0.01, R.LrSchedule("cosine", 2, 0.005), 0.9)
    assert R.check_optim_options(ok) == R.check_optim_options(ok, flat_path=True)
    # --lr_decay goes with weight decay and the EMA: only a second SCHEDULE is refused
    R.check_optim_options(Namespace(lr=5e-3, weight_decay=0.01, ema=0.9, lr_decay=True), flat_path=True)


@pytest.mark.parametrize("flag", [dict(weight_decay=0.01), dict(lr_schedule="constant"), dict(ema=0.5)])
def test_no_flat_path_no_flag(flag):
    """there is no CPU optimizer twin: check_args (a machine without a GPU) and Experiment (a CPU device) refuse each flag"""
    import speech_imagery_eeg_amd  # noqa: F401
    import run
    from exp.experiment_classification import Experiment
    R = _rule()
    with pytest.raises(ValueError, match="flat optimizer path"):
        R.check_optim_options(Namespace(lr=5e-3, **flag), flat_path=False)
    e = Experiment.__new__(Experiment)
    e.args, e.device, e.rank = Namespace(lr=5e-3, **flag), torch.device("cpu"), 0
    with pytest.raises(ValueError, match="flat optimizer path"):
        e._resolve_optim_options()
    if not torch.cuda.is_available():
        argv = [a for k, v in flag.items() for a in ("--" + k, str(v))]
        with pytest.raises(ValueError, match="flat optimizer path"):
            run.get_args(SYNTH + argv)


def test_experiment_refuses_for_callers_that_build_the_namespace_themselves():
    import speech_imagery_eeg_amd  # noqa: F401
    from exp.experiment_classification import Experiment
    from exp.experiment_regression import Experiment as Regression
    for cls in (Experiment, Regression):
        e = cls.__new__(cls)
        e.device, e.rank = torch.device("cuda"), 0
        for bad, match in ((dict(lr_schedule="cosine", lr_decay=True), "lr_decay"), (dict(ema=0.9, shapelet_project=3), "shapelet_project"),
                           (dict(ema=1.5), "ema"), (dict(weight_decay=-1.0), "weight_decay"), (dict(lr_schedule="cosine,min=1"), "above")):
            e.args = Namespace(lr=5e-3, **bad)
            with pytest.raises(ValueError, match=match):
                e._resolve_optim_options()
        e.args = Namespace(lr=5e-3)
        e._resolve_optim_options()
        assert e._optim_active is False and e._ema is False
        e.args = Namespace(lr=5e-3, ema=0.9, shapelet_project="end")
        e._resolve_optim_options()
        assert e._optim_active and e._ema


def test_total_steps_counts_the_closing_steps_of_the_run_wide_count():
    R = _rule()
    assert R.total_steps(2, 3) == 6 and R.total_steps(2, 3, 2) == 3 and R.total_steps(3, 5, 4) == 3 and R.total_steps(1, 3, 4) == 0
    for epochs, batches, K in ((2, 3, 2), (3, 5, 4), (2, 6, 2), (1, 3, 4)):
        assert R.total_steps(epochs, batches, K) == sum(1 for step in range(1, epochs * batches + 1) if step % K == 0)


# ---------------------------------------------------------------- the schedule
def _closed_form(kind, W, S, s, floor):
    if s < W:
        return BASE * s / W
    if kind == "constant":
        return BASE
    T = max(1, S - W)
    return floor + (BASE - floor) * 0.5 * (1.0 + math.cos(math.pi * min(s - W, T) / T))


@pytest.mark.parametrize("W,S", CASES)
def test_lr_at_pin(W, S):
    R = _rule()
    for floor in (0.0, FLOOR):
        spec = R.LrSchedule("cosine", W, floor)
        got = [R.lr_at(spec, BASE, S, s) for s in range(1, S + 4)]
        if W == 0:
            # torch's scheduler in float64 on the CPU: after s scheduler steps the optimizer holds the rate of update s + 1 of a run
            # that starts at base, i.e. lr(s) of the rule; torch recurs from step to step, so the two agree to a few ulp per step
            opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))], lr=BASE)
            sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=max(1, S), eta_min=floor)
            for s in range(1, S + 1):
                opt.step()
                sched.step()
                assert abs(got[s - 1] - opt.param_groups[0]["lr"]) <= 1e-12 * BASE, (s, got[s - 1], opt.param_groups[0]["lr"])
        for s in range(1, S + 4):
            assert got[s - 1] == _closed_form("cosine", W, S, s, floor), s
        assert all(floor * (s >= W) <= v <= BASE * (1 + 1e-15) for s, v in enumerate(got[:S], 1))
        if 0 < W <= S:
            assert abs(R.lr_at(spec, BASE, S, W) - BASE) <= 1e-15 * BASE                           # lr(W) = base
        if W < S:
            assert abs(R.lr_at(spec, BASE, S, S) - floor) <= 1e-15 * BASE                          # lr(S) = M
            assert got[S:] == [got[S - 1]] * 3               # past the run's end the rate stays at its last value
    const = R.LrSchedule("constant", W, 0.0)
    assert [R.lr_at(const, BASE, S, s) for s in range(1, S + 4)] == [_closed_form("constant", W, S, s, 0.0) for s in range(1, S + 4)]
    assert [R.lr_at(R.LrSchedule(), BASE, S, s) for s in (1, 2, S + 3)] == [BASE] * 3


def test_warmup_longer_than_the_run_never_reaches_base():
    R = _rule()
    spec = R.LrSchedule("cosine", 5, FLOOR)
    assert [R.lr_at(spec, BASE, 4, s) for s in (1, 2, 3, 4)] == [BASE * s / 5 for s in (1, 2, 3, 4)]


def test_ema_decay_warms_up():
    R = _rule()
    assert [R.ema_decay_at(0.999, s) for s in range(1, 6)] == [2 / 11, 3 / 12, 4 / 13, 5 / 14, 6 / 15]
    assert R.ema_decay_at(0.3, 1) == 2 / 11 and R.ema_decay_at(0.3, 3) == 0.3 and R.ema_decay_at(0.999, 10 ** 6) == 0.999
    p = np.array([1.0, -2.0, 3.5])
    assert np.array_equal(R.ema_reference(p, p, 0.9, 4), p)


# ---------------------------------------------------------------- AdamW
def test_adamw_reference_equals_torch_adamw_in_float64():
    R = _rule()
    rng = np.random.default_rng(0)
    p, m, v = rng.standard_normal(257), np.zeros(257), np.zeros(257)
    q = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.AdamW([q], lr=5e-3, weight_decay=0.05)
    for step in range(1, 6):
        g = rng.standard_normal(257)
        q.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = R.adamw_reference(p, g, m, v, lr=5e-3, step=step, weight_decay=0.05)
        assert float(np.abs(p - q.detach().numpy()).max()) <= 1e-12, step
    assert float(np.abs(m - opt.state[q]["exp_avg"].numpy()).max()) <= 1e-12
    assert float(np.abs(v - opt.state[q]["exp_avg_sq"].numpy()).max()) <= 1e-12


def test_adamw_reference_mask_and_zero_decay():
    R = _rule()
    rng = np.random.default_rng(1)
    p, g, m, v = rng.standard_normal(10), rng.standard_normal(10), rng.standard_normal(10), rng.random(10)
    plain = R.adamw_reference(p, g, m, v, lr=1e-2, step=3)
    assert all(np.array_equal(a, b) for a, b in zip(plain, R.adamw_reference(p, g, m, v, lr=1e-2, step=3, weight_decay=0.1,
                                                                             decay=np.zeros(10, bool))))
    half = np.arange(10) < 5
    mixed = R.adamw_reference(p, g, m, v, lr=1e-2, step=3, weight_decay=0.1, decay=half)[0]
    full = R.adamw_reference(p, g, m, v, lr=1e-2, step=3, weight_decay=0.1)[0]
    assert np.array_equal(mixed[:5], full[:5]) and np.array_equal(mixed[5:], plain[0][5:]) and not np.array_equal(full, plain[0])


# ---------------------------------------------------------------- which parameters decay
def _models():
    import speech_imagery_eeg_amd  # noqa: F401
    from models.eegcnn import EEGCNNTransformer
    from models.InterpGN import InterpGN, dnn_dict
    from models.Shapelet import DistThresholdSBM, ShapeBottleneckModel
    lens = [0.05, 0.1, 0.2, 0.3, 0.5, 0.8]
    torch.manual_seed(0)
    return {"InterpGN": InterpGN(make_cfg()),
            "SBM": ShapeBottleneckModel(make_cfg(), [3] * 6, lens),
            "LTS": DistThresholdSBM(make_cfg(), [3] * 6, lens),
            "Transformer": dnn_dict["Transformer"](make_cfg(dnn_type="Transformer")),
            "EEGCNN": EEGCNNTransformer(make_cfg(enc_in=8, seq_len=200, num_class=3, c_out=3, d_model=128))}


def test_decays_on_the_models():
    R = _rule()
    from models.Shapelet import Shapelet
    for tag, model in _models().items():
        named = dict(model.named_parameters())
        verdict = {k: R.decays(k, p) for k, p in named.items()}
        assert any(verdict.values()) and not all(verdict.values()), tag
        for k, p in named.items():
            if p.ndim < 2:
                assert not verdict[k], (tag, k)               # biases, BatchNorm / LayerNorm affine parameters
        banks = 0
        for name, mod in model.named_modules():
            prefix = name + "." if name else ""
            if isinstance(mod, Shapelet):
                banks += 1
                assert not verdict[prefix + "weights"], (tag, name)
                if hasattr(mod, "threshold"):
                    assert mod.threshold.ndim >= 2 and not verdict[prefix + "threshold"], (tag, name)
            if isinstance(mod, (torch.nn.Linear, torch.nn.Conv1d, torch.nn.Conv2d)):
                assert verdict[prefix + "weight"], (tag, name)
                if mod.bias is not None:
                    assert not verdict[prefix + "bias"], (tag, name)
            if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d, torch.nn.LayerNorm)) and mod.weight is not None:
                assert not verdict[prefix + "weight"] and not verdict[prefix + "bias"], (tag, name)
        assert (banks > 0) == (tag in ("InterpGN", "SBM", "LTS")), tag
        if tag == "LTS":
            assert sum(k.endswith("threshold") for k in named) == banks


def test_decay_mask_is_one_byte_per_chunk_of_a_decaying_parameter():
    R = _rule()
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip.ddp import FlatParamBucket
    net = torch.nn.Sequential(torch.nn.Linear(13, 10), torch.nn.BatchNorm1d(10), torch.nn.Linear(10, 7))
    bucket = FlatParamBucket(net, 1)                    # weight 130 (3 chunks), bias 10, bn 10 + 10, weight 70 (2 chunks), bias 7
    assert bucket.offsets == [0, 192, 256, 320, 384, 512] and bucket.flat_grad.numel() == 576
    names = [k for k, _ in net.named_parameters()]
    mask = R.decay_mask(names, bucket.params, bucket.offsets, 576, bucket.ALIGN)
    assert mask.dtype == np.uint8 and mask.tolist() == [1, 1, 1, 0, 0, 0, 1, 1, 0]
    with pytest.raises(ValueError, match="multiple of 64"):
        R.decay_mask(names, bucket.params, [o + 4 for o in bucket.offsets], 600)


# ---------------------------------------------------------------- FlatAdam's host path against a stand-in library
class _StandIn:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 4096 if name.endswith("_bytes") else 0
        return fn


def _header_params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    m = re.search(r"\b(int|float|size_t)\s+" + name + r"\s*\(([^)]*)\)", hdr)
    assert m, f"{name} is not declared in include/ign_abi.h"
    out = []
    for p in m.group(2).split(","):
        p = " ".join(p.split())
        pname = re.split(r"[\s*]+", p)[-1]
        out.append((p[:len(p) - len(pname)].strip(), pname))
    return m.group(1), out


def _val(a):
    if a is None or isinstance(a, (int, float)):
        return a
    return a.value if isinstance(a, ctypes.c_void_p) else a.data_ptr()


def _named(call, name):
    got, args = call
    assert got == name
    params = [p for _, p in _header_params(name)[1]]
    assert len(args) == len(params), name
    return dict(zip(params, [_val(a) for a in args]))


@pytest.fixture
def host(monkeypatch):
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ddp
    rec = _StandIn()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "check", lambda rc, what: None)
    monkeypatch.setattr(_lib, "stream", lambda: ctypes.c_void_p(0x5EED))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    return _lib, ddp, rec


def _net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 2))


def _opt(ddp, **kw):
    """FlatAdam over a fresh bucket, every parameter with a gradient autograd would have left"""
    bucket = ddp.FlatParamBucket(_net(), 1)
    opt = ddp.FlatAdam(bucket, **kw)
    for i, p in enumerate(bucket.params):
        p.grad = torch.full_like(p, float(i + 1))
    return bucket, opt


@pytest.mark.parametrize("clip", [False, True])
def test_scheduled_flat_adam_calls_the_one_adamw_entry_point(host, clip):
    _lib, ddp, rec = host
    bucket, opt = _opt(ddp, lr=5e-3, weight_decay=0.01, schedule="cosine,warmup=2,min=1e-4", total_steps=9, ema=0.9)
    assert opt.scheduled and opt.capturable and opt.hp_dev.numel() == 4 and opt.step_dev.dtype == torch.int32
    assert opt.bc_dev.data_ptr() == opt.hp_dev.data_ptr()
    assert opt.decay_mask.dtype == torch.uint8 and opt.decay_mask.tolist() == [1, 0, 1, 0]
    assert torch.equal(opt.ema_flat, opt.flat_param) and opt.ema_flat.data_ptr() != opt.flat_param.data_ptr()
    rec.calls.clear()
    gen = _lib.PARAM_GENERATION[0]
    opt.step(max_norm=0.5 if clip else None)
    names = [c[0] for c in rec.calls]
    assert names == ["ign_gather_flat"] + (["ign_grad_norm_workspace_bytes", "ign_grad_norm_clip"] if clip else []) + ["ign_adamw_step_dev"]
    a = _named(rec.calls[-1], "ign_adamw_step_dev")
    assert a["param"] == opt.flat_param.data_ptr() and a["grad"] == bucket.flat_grad.data_ptr() and a["n"] == 256
    assert a["exp_avg"] == opt.exp_avg.data_ptr() and a["exp_avg_sq"] == opt.exp_avg_sq.data_ptr()
    assert (a["beta1"], a["beta2"], a["eps"], a["weight_decay"]) == (0.9, 0.999, 1e-8, 0.01)
    assert a["decay_mask"] == opt.decay_mask.data_ptr()
    assert (a["sched_kind"], a["base_lr"], a["warmup"], a["min_lr"], a["total_steps"], a["ema_decay"]) == (1, 5e-3, 2, 1e-4, 9, 0.9)
    assert a["step_dev"] == opt.step_dev.data_ptr() and a["hp_dev"] == opt.hp_dev.data_ptr() and a["stream"] == 0x5EED
    assert a["coef_dev"] == (opt.norm_dev.data_ptr() + 4 if clip else None)
    assert opt.step_count == 0 and _lib.PARAM_GENERATION[0] == gen + 1       # no host count beside step_dev
    rec.calls.clear()
    opt.ema_update()
    e = _named(rec.calls[0], "ign_ema_update")
    assert (e["ema"], e["param"], e["n"], e["hp_dev"]) == (opt.ema_flat.data_ptr(), opt.flat_param.data_ptr(), 256, opt.hp_dev.data_ptr())
    opt.swap_ema()
    s = _named(rec.calls[1], "ign_swap_flat")
    assert (s["a"], s["b"], s["n"]) == (opt.flat_param.data_ptr(), opt.ema_flat.data_ptr(), 256)
    assert _lib.PARAM_GENERATION[0] == gen + 2                               # ops.py's caches of parameter-derived values
    assert opt.lr_at(1) == 5e-3 / 2 and opt.lr_at(2) == 5e-3 and abs(opt.lr_at(9) - 1e-4) < 1e-18


def test_each_option_alone_selects_the_adamw_path_and_neutral_settings_do_not(host):
    _lib, ddp, rec = host
    for kw, mask, ema in ((dict(weight_decay=0.1), True, False), (dict(schedule="constant"), False, False),
                          (dict(schedule="constant,warmup=3"), False, False), (dict(ema=0.5), False, True)):
        opt = _opt(ddp, lr=1e-3, **kw)[1]
        assert opt.scheduled and opt.capturable
        assert (opt.decay_mask is not None) == mask and (opt.ema_flat is not None) == ema
        rec.calls.clear()
        opt.step()
        assert [c[0] for c in rec.calls] == ["ign_gather_flat", "ign_adamw_step_dev"]
        assert _named(rec.calls[1], "ign_adamw_step_dev")["decay_mask"] == (opt.decay_mask.data_ptr() if mask else None)
    for kw in ({}, dict(weight_decay=0.0, schedule="none", total_steps=7, ema=0.0), dict(schedule=None)):
        opt = _opt(ddp, lr=1e-3, **kw)[1]
        assert not opt.scheduled and not opt.capturable and opt.hp_dev is None and opt.ema_flat is None and opt.decay_mask is None
        rec.calls.clear()
        opt.step()
        assert [c[0] for c in rec.calls] == ["ign_gather_flat", "ign_adam_step"] and opt.step_count == 1
        with pytest.raises(_lib.IgnError):
            opt.ema_update()
        with pytest.raises(_lib.IgnError):
            opt.swap_ema()
    with pytest.raises(ValueError, match="total_steps"):
        ddp.FlatAdam(ddp.FlatParamBucket(_net(), 1), lr=1e-3, schedule="cosine")
    with pytest.raises(ValueError):
        ddp.FlatAdam(ddp.FlatParamBucket(_net(), 1), lr=1e-3, ema=1.0)


# ---------------------------------------------------------------- the C side
def test_new_symbols_are_declared_bound_and_exported():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    types = {"int": _lib.ci, "float": _lib.cf, "double": _lib.cd, "long long": _lib.ll, "size_t": _lib.sz}
    for name in NEW:
        res, params = _header_params(name)
        assert name in _lib.SIGNATURES, name
        bres, bargs = _lib.SIGNATURES[name]
        assert bres is types[res], name
        assert [(_lib.vp if "*" in t else types[t]) for t, _ in params] == list(bargs), (name, params)
    assert _header_params("ign_adamw_step_dev")[1][-2:] == [("const float*", "coef_dev"), ("void*", "stream")]
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so is not built")
    h = ctypes.CDLL(_lib.lib_path())
    for name in NEW:
        assert hasattr(h, name), f"{name} is not exported"
    assert _lib.lib().ign_abi_version() == 1


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("W,S", CASES)
def test_ign_sched_lr_is_the_numpy_rule(W, S):
    L, R = _lib_or_skip(), _rule()
    for kind in ("constant", "cosine"):
        for floor in (0.0, FLOOR):
            spec = R.LrSchedule(kind, W, floor if kind == "cosine" else 0.0)
            for s in range(1, S + 4):
                got, want = L.ign_sched_lr(spec.code, BASE, W, spec.min_lr, S, s), np.float32(R.lr_at(spec, BASE, S, s))
                if kind == "constant" or s < W:
                    assert np.float32(got) == want, (kind, s)              # base * s / W and base: the same IEEE operations
                else:
                    assert _ulps(got, want) <= 1, (kind, s, got, want)     # two double-precision cos may differ in the last place


def _p(addr):
    return ctypes.c_void_p(0x10000 + addr)


@pytest.mark.parametrize("kw,msg", [
    (dict(param=None), b"null pointer"), (dict(grad=None), b"null pointer"), (dict(exp_avg=None), b"null pointer"),
    (dict(exp_avg_sq=None), b"null pointer"), (dict(step_dev=None), b"null pointer"), (dict(hp_dev=None), b"null pointer"),
    (dict(n=0), b"n <= 0"), (dict(n=-4), b"n <= 0"),
    (dict(param=_p(4)), b"16-byte"), (dict(grad=_p(8)), b"16-byte"), (dict(exp_avg=_p(12)), b"16-byte"), (dict(exp_avg_sq=_p(1)), b"16-byte"),
    (dict(sched_kind=2), b"out of range"), (dict(warmup=-1), b"out of range"), (dict(min_lr=-1e-4), b"out of range"),
    (dict(min_lr=1.0), b"out of range"), (dict(weight_decay=-0.1), b"out of range"), (dict(ema_decay=1.0), b"out of range"),
    (dict(ema_decay=-0.5), b"out of range"), (dict(total_steps=-1), b"out of range"), (dict(base_lr=float("nan")), b"out of range"),
])
def test_adamw_step_refuses_bad_arguments_before_any_launch(kw, msg):
    L = _lib_or_skip()
    a = dict(param=_p(0), grad=_p(0x100), exp_avg=_p(0x200), exp_avg_sq=_p(0x300), n=8, beta1=0.9, beta2=0.999, eps=1e-8,
             weight_decay=0.01, decay_mask=None, sched_kind=1, base_lr=5e-3, warmup=2, min_lr=1e-4, total_steps=5, ema_decay=0.9,
             step_dev=_p(0x400), hp_dev=_p(0x500), coef_dev=None, stream=None)
    assert list(a) == [p for _, p in _header_params("ign_adamw_step_dev")[1]]
    a.update(kw)
    assert L.ign_adamw_step_dev(*a.values()) == E_ARG
    assert msg in L.ign_last_error() and b"ign_adamw_step_dev" in L.ign_last_error()


@pytest.mark.parametrize("kw,msg", [(dict(ema=None), b"null pointer"), (dict(param=None), b"null pointer"), (dict(hp_dev=None), b"null pointer"),
                                    (dict(n=0), b"n <= 0"), (dict(ema=_p(4)), b"16-byte"), (dict(param=_p(8)), b"16-byte")])
def test_ema_update_refuses_bad_arguments_before_any_launch(kw, msg):
    L = _lib_or_skip()
    a = dict(ema=_p(0), param=_p(0x100), n=8, hp_dev=_p(0x200), stream=None)
    assert list(a) == [p for _, p in _header_params("ign_ema_update")[1]]
    a.update(kw)
    assert L.ign_ema_update(*a.values()) == E_ARG
    assert msg in L.ign_last_error() and b"ign_ema_update" in L.ign_last_error()


@pytest.mark.parametrize("kw,msg", [(dict(a=None), b"null pointer"), (dict(b=None), b"null pointer"), (dict(n=0), b"n <= 0"),
                                    (dict(n=-1), b"n <= 0"), (dict(a=_p(4)), b"16-byte"), (dict(b=_p(0x108)), b"16-byte"),
                                    (dict(b=_p(0)), b"overlap"), (dict(b=_p(16)), b"overlap"), (dict(a=_p(0x110)), b"overlap")])
def test_swap_flat_refuses_bad_arguments_before_any_launch(kw, msg):
    L = _lib_or_skip()
    a = dict(a=_p(0), b=_p(0x100), n=8, stream=None)
    assert list(a) == [p for _, p in _header_params("ign_swap_flat")[1]]
    a.update(kw)
    assert L.ign_swap_flat(*a.values()) == E_ARG
    assert msg in L.ign_last_error() and b"ign_swap_flat" in L.ign_last_error()
