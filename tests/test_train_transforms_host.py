"""The chain of the training-batch transforms (utils/train_transforms.py) on the host, no GPU: every on / off subset of --warp,
--augment and --mix in both training loops against recording stand-in ops (which ran, in which order, one mask sum and one step
seed per step, one lengths tensor for all stages), the regression refusal from both places with one wording, the recorded table of
what the three parsers accept and refuse (tests/golden/train_flag_refusals.json, taken before they moved onto FlagItems), and the
checks the three launchers share (csrc/ign_btc.h), which return before any launch.  The GPU side is tests/test_gpu_train_transforms.py."""
import ctypes
import itertools
import json
import os
from argparse import Namespace

import pytest
import torch

from conftest import ROOT

import speech_imagery_eeg_amd  # noqa: F401
from utils import train_transforms as TT
from utils.augment import step_seed

FLAGS = dict(warp="twarp=0.2,mwarp=0.1,knots=3", augment="shift=0.1,time_mask=0.2", mix="mixup=0.4,cutmix=1")
SUBSETS = [s for r in range(4) for s in itertools.combinations(TT.ORDER, r)]
E_ARG, E_TOOBIG = -1001, -1003


class _Stop(Exception):
    pass


class _Mask:
    """Stands in for the keep-mask: counts its row sums."""

    def __init__(self, mask):
        self.mask, self.sums = mask, 0

    def sum(self, dim):
        self.sums += 1
        return self.mask.sum(dim)


def _bare_experiment(monkeypatch, order, graphed, flags):
    """An Experiment with nothing behind it but what the two training loops touch before the forward pass, which stops the loop
    (as tests/test_warp_host.py); the three ops are recording stand-ins and step_seed counts its calls."""
    from exp import experiment_classification as E

    def op(name):
        def fn(x, *a, **k):
            order.append((name, a, k))
            return x + 1.0
        return fn
    for name in TT.ORDER:
        monkeypatch.setattr(E.ign_ops, name, op(name))
    seeds = []

    def counted_seed(base, rank, step):
        seeds.append((base, rank, step))
        return step_seed(base, rank, step)
    monkeypatch.setattr(TT, "step_seed", counted_seed)
    e = object.__new__(E.Experiment)
    e.args = Namespace(amp=False, gradient_accumulation_steps=1, seed=11, batch_size=999, model="SBM", train_epochs=2,
                       beta_schedule="constant", task_name="classification", **flags)
    e.rank, e.device, e.distributed = 3, torch.device("cpu"), False
    e.model = torch.nn.Identity()
    e.optimizer = Namespace(schedule=Namespace(active=True), capturable=True)
    B, T, C = 4, 12, 2
    keep = torch.ones(B, T)
    keep[1, 7:] = 0
    mask = _Mask(keep)
    e.train_loader = [(torch.zeros(B, T, C), torch.arange(B) % 2, mask)] * 2
    e._to_device = lambda x, y, m: (x, y, m)
    e._graph_eligible = lambda amp: graphed

    def forward(batch_x, padding_mask):
        order.append(("forward", (float(batch_x.mean()),), {}))
        raise _Stop
    e._forward = forward
    e._resolve_train_transforms()
    return e, mask, seeds


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "hipgraph"])
@pytest.mark.parametrize("on", SUBSETS, ids=["+".join(s) or "nothing" for s in SUBSETS])
def test_every_subset_runs_its_stages_in_order_with_one_mask_sum_and_one_seed(monkeypatch, on, graphed):
    order = []
    e, mask, seeds = _bare_experiment(monkeypatch, order, graphed, {name: FLAGS[name] for name in on})
    chain = e._transforms
    assert bool(chain) == bool(on) and [name for name in TT.ORDER if getattr(chain, name) is not None] == list(on)
    assert chain.base == (11 if on else None)
    with pytest.raises(_Stop):
        e.train_one_epoch(0, 40)
    assert [o[0] for o in order] == list(on) + ["forward"]
    assert order[-1][1] == (float(len(on)),)                          # each stand-in added 1: the forward saw every stage that is on
    assert mask.sums == (1 if on else 0) and seeds == ([(11, 3, 41)] if on else [])
    lengths = [o[2]["lengths"] for o in order[:-1]]
    assert all(n is lengths[0] for n in lengths)                     # one tensor for every stage
    if on:
        assert lengths[0].dtype == torch.int32 and lengths[0].tolist() == [12, 7, 12, 12]
    for name, a, k in order[:-1]:
        if name != "mix":
            assert a == (step_seed(11, 3, 41),) and set(k) == {"lengths"} | set(getattr(chain, name)._fields)
        else:
            assert set(k) == {"span", "lengths"} and len(a) == 2 and k["span"].dtype == torch.int32    # (lam, roll); cutmix: a span
    # the call itself
    x, label = torch.zeros(4, 12, 2), torch.arange(4) % 2
    out, soft = chain(x, label, mask if on else None, 41)
    if not on:
        assert out is x and soft == ()                               # nothing is touched: the mask is not even looked at
    elif "mix" in on:
        from utils.mix import mix_draws
        roll, lam, _ = mix_draws(step_seed(11, 3, 41), 4, [12, 7, 12, 12], chain.mix)
        assert torch.equal(soft[0], label.roll(-roll)) and torch.equal(soft[1], torch.from_numpy(lam))
        assert order[-1][1][0] is soft[1] and order[-1][1][1] == roll
    else:
        assert soft == ()


def test_regression_refusal_has_one_wording():
    import run
    words = []
    for raise_it in (lambda: run.get_args(["--data", "SYNTH", "--task_name", "regression", "--mix", "mixup=0.4"]),
                     lambda: TT.parse_flags(Namespace(mix="mixup=0.4", task_name="regression")),
                     lambda: TT.TrainTransforms.from_args(Namespace(mix="cutmix=1", task_name="regression", seed=0), rank=1)):
        with pytest.raises(ValueError, match="--mix with --task_name regression") as err:
            raise_it()
        words.append(str(err.value))
    assert len(set(words)) == 1
    src = "".join(open(os.path.join(ROOT, "speech-imagery-eeg_amd", *p)).read() for p in (("run.py",), ("exp", "experiment_classification.py")))
    assert "CRPS tails have no soft-label form" not in src            # stated once, in the chain module
    chain = TT.TrainTransforms.from_args(Namespace(mix="none", warp="twarp=0.2", augment="noise=0.1", task_name="regression", seed=0))
    assert chain.mix is None and chain.warp is not None and chain.augment is not None


# ---------------------------------------------------------------- the recorded table of the three parsers
with open(os.path.join(ROOT, "tests", "golden", "train_flag_refusals.json")) as _f:
    TABLE = json.load(_f)
ROWS = [(flag, row) for flag in TT.ORDER for row in TABLE[flag]]


def _parser(flag):
    return getattr(TT._MODULES[flag], "parse_" + flag)


def test_the_table_covers_what_it_has_to():
    for flag in TT.ORDER:
        texts = [row["text"] for row in TABLE[flag]]
        assert {None, "", "none", "NONE", " none "} <= set(texts)
        errors = [row["error"] for row in TABLE[flag] if "error" in row]
        for part in ("is not one of", "given twice", "is not a number"):
            assert any(part in e for e in errors), (flag, part)
    aug = {row["text"] for row in TABLE["augment"]}
    assert {"shift", "shift=", "shift=nan", "noise=inf", "shift=1", "noise=-0", "chan_drop=0.99999"} <= aug
    mix = {row["text"] for row in TABLE["mix"]}
    assert {"mixup", "mixup=", "mixup=nan", "mixup=inf", "mixup=0", "prob=0", "prob=1", "prob="} <= mix


@pytest.mark.parametrize("flag,row", ROWS, ids=[f"{flag}:{row['text']!r}" for flag, row in ROWS])
def test_every_recorded_answer_reproduces(flag, row):
    text = row["text"]
    if "error" in row:
        for parse in (_parser(flag), lambda t: TT.parse_flags(Namespace(**{flag: t}))):
            with pytest.raises(ValueError) as err:
                parse(text)
            assert str(err.value) == row["error"]
        return
    spec = _parser(flag)(text)
    assert {k: repr(v) for k, v in spec._asdict().items()} == {k: repr(v) for k, v in row["spec"].items()}     # field by field, -0.0 too
    assert TT.parse_flags(Namespace(**{flag: text}))[flag] == (spec if spec.active else None)


@pytest.mark.parametrize("flag", TT.ORDER)
def test_none_never_reaches_a_parser(monkeypatch, flag):
    def refuse(spec):
        raise AssertionError(f"--{flag} none must not reach the parser")
    monkeypatch.setattr(TT._MODULES[flag], "parse_" + flag, refuse)
    for text in (None, "", "none", "None", " NONE ", "\tnone\n"):
        assert TT.parse_flags(Namespace(**{flag: text}))[flag] is None
    assert TT.parse_flags(Namespace()) == dict.fromkeys(TT.ORDER)     # a namespace without the flags
    assert not TT.TrainTransforms.from_args(Namespace())
    with pytest.raises(AssertionError):
        TT.parse_flags(Namespace(**{flag: FLAGS[flag]}))


# ---------------------------------------------------------------- the launchers' shared checks
def _entry_points(h):
    def augment(x, out, B, T, C):
        return h.ign_augment_btc(x, out, None, B, T, C, 7, 0.1, 0.0, 0.0, 0, 0.0, None)

    def warp(x, out, B, T, C):
        return h.ign_warp_btc(x, out, None, B, T, C, 7, 0.2, 0.1, 0.1, 4, 1.0, None)

    def mix(x, out, B, T, C):
        return h.ign_mix_btc(x, out, None, ctypes.c_void_p(64), None, 1, B, T, C, None)
    return {"ign_augment_btc": augment, "ign_warp_btc": warp, "ign_mix_btc": mix}


@pytest.mark.parametrize("name", ["ign_augment_btc", "ign_warp_btc", "ign_mix_btc"])
def test_launchers_share_their_refusals_without_a_device(name):
    """every refusal returns before a launch: the pointers are not device memory and no GPU is needed to run this"""
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    h = _lib.lib()
    call = _entry_points(h)[name]
    P, Q, FAR = 1 << 20, 1 << 24, 1 << 60
    p = ctypes.c_void_p
    B, T, C = 2, 8, 3
    cases = [("null x", (None, p(Q), B, T, C), E_ARG, b"null"), ("null out", (p(P), None, B, T, C), E_ARG, b"null"),
             ("B = 0", (p(P), p(Q), 0, T, C), E_ARG, b"non-positive"), ("T = 0", (p(P), p(Q), B, 0, C), E_ARG, b"non-positive"),
             ("C = 0", (p(P), p(Q), B, T, 0), E_ARG, b"non-positive"),
             ("x == out", (p(P), p(P), B, T, C), E_ARG, b"overlap"),
             ("out at the last element of x", (p(P), p(P + 4 * (B * T * C - 1)), B, T, C), E_ARG, b"overlap"),
             ("x one element inside out", (p(Q + 4), p(Q), B, T, C), E_ARG, b"overlap"),
             ("T * C beyond a 32-bit index", (p(P), p(FAR), B, 1 << 20, 1 << 11), E_TOOBIG, b"32-bit index"),
             ("more blocks than a grid has", (p(P), p(FAR), 1 << 30, 8192, 1), E_TOOBIG, b"more blocks")]
    for what, args, code, word in cases:
        assert call(*args) == code, what
        msg = h.ign_last_error()
        assert name.encode() in msg and word in msg, (what, msg)
    # the buffer right behind x does not overlap it (the next check refuses the grid); one element earlier it does
    B, T, C = 1 << 30, 8192, 1
    assert call(p(P), p(P + 4 * B * T * C), B, T, C) == E_TOOBIG and b"more blocks" in h.ign_last_error()
    assert call(p(P), p(P + 4 * B * T * C - 4), B, T, C) == E_ARG and b"overlap" in h.ign_last_error()
