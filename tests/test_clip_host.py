"""Gradient clipping and accumulation on the flat gradient buffer, host side: the bindings of the new entry points against
include/ign_abi.h, which entry points FlatAdam.step / FlatParamBucket.gather call and with which arguments, the `_dirty` / `p.grad`
bookkeeping of the accumulating gather, and the `--hipgraph` eligibility rule.  Needs neither a device nor libign_hip.so: the host
code runs on CPU tensors that claim to be on the GPU, against a stand-in library that records the calls."""
import ctypes
import os
import re
from argparse import Namespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM = 0x5EED
NEW = ("ign_grad_norm_workspace_bytes", "ign_grad_norm_clip", "ign_adam_step_clip", "ign_adam_step_clip_dev", "ign_scale_flat",
       "ign_gather_flat_acc")


def _mods():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ddp
    return _lib, ddp


def _header_params(name):
    """[(type text, parameter name)] of `name` as include/ign_abi.h declares it"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^)]*)\)", hdr)
    assert m, name
    out = []
    for p in m.group(2).split(","):
        p = " ".join(p.split())
        pname = re.split(r"[\s*]+", p)[-1]
        out.append((p[:len(p) - len(pname)].strip(), pname))
    return m.group(1), out


def _ctype(_lib, text):
    if "*" in text:
        return _lib.vp
    return {"int": _lib.ci, "float": _lib.cf, "long long": _lib.ll, "size_t": _lib.sz}[text]


@pytest.mark.parametrize("name", NEW)
def test_lib_binds_the_new_symbols_with_the_headers_argument_lists(name):
    _lib, _ = _mods()
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    hres, hparams = _header_params(name)
    assert res is _ctype(_lib, hres)
    assert [_ctype(_lib, t) for t, _ in hparams] == list(args), (name, hparams)


def test_clip_entry_points_are_the_existing_ones_plus_the_coefficient_pointer():
    for old, new in (("ign_adam_step", "ign_adam_step_clip"), ("ign_adam_step_dev", "ign_adam_step_clip_dev")):
        a, b = _header_params(old)[1], _header_params(new)[1]
        assert b[:len(a) - 1] == a[:-1] and b[-1] == a[-1] and b[-2] == ("const float*", "coef_dev")
    assert _header_params("ign_gather_flat_acc")[1] == _header_params("ign_gather_flat")[1]


# ---------------------------------------------------------------- stand-in library
class _StandIn:
    """Every attribute is an entry point that records (name, args); size queries answer `nbytes`, launches 0."""

    def __init__(self, nbytes=4096):
        self.calls, self.nbytes = [], nbytes

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return self.nbytes if name.endswith("_bytes") else 0
        return fn


def _val(a):
    if a is None or isinstance(a, (int, float)):
        return a
    if isinstance(a, ctypes.c_void_p):
        return a.value
    if isinstance(a, ctypes.Array):
        return list(a)
    return a.data_ptr()


def _named(_lib, call, name):
    """The recorded call as {header parameter name: value}; the argument count is the signature's and the header's."""
    got, args = call
    assert got == name
    params = [p for _, p in _header_params(name)[1]]
    assert len(args) == len(_lib.SIGNATURES[name][1]) == len(params), name
    return dict(zip(params, [_val(a) for a in args]))


@pytest.fixture
def host(monkeypatch):
    """The GPU host path on CPU tensors: tensors answer is_cuda = True, the library is the recorder."""
    _lib, ddp = _mods()
    rec = _StandIn()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "check", lambda rc, what: None)
    monkeypatch.setattr(_lib, "stream", lambda: ctypes.c_void_p(STREAM))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    return _lib, ddp, rec


def _net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 2))        # 4 parameters: 15, 5, 10, 2 floats


def _set_grads(net, skip=()):
    for i, p in enumerate(net.parameters()):
        p.grad = None if i in skip else torch.full_like(p, float(i + 1))


@pytest.mark.parametrize("capturable", [False, True])
def test_step_with_max_norm_calls_the_norm_once_then_the_clip_adam_with_the_coefficient(host, capturable):
    _lib, ddp, rec = host
    net = _net()
    bucket = ddp.FlatParamBucket(net, 1)
    opt = ddp.FlatAdam(bucket, lr=1e-3, capturable=capturable)
    _set_grads(net)
    rec.calls.clear()
    opt.step(max_norm=0.5)
    adam = "ign_adam_step_clip_dev" if capturable else "ign_adam_step_clip"
    assert [c[0] for c in rec.calls] == ["ign_gather_flat", "ign_grad_norm_workspace_bytes", "ign_grad_norm_clip", adam]
    norm = _named(_lib, rec.calls[2], "ign_grad_norm_clip")
    assert norm["g"] == bucket.flat_grad.data_ptr() and norm["n"] == bucket.flat_grad.numel() and norm["max_norm"] == 0.5
    assert norm["out2"] == opt.norm_dev.data_ptr() and norm["workspace"] and norm["stream"] == STREAM
    step = _named(_lib, rec.calls[3], adam)
    assert step["coef_dev"] == opt.norm_dev.data_ptr() + 4                           # non-null: out2[1], the coefficient
    assert step["grad"] == bucket.flat_grad.data_ptr() and step["param"] == opt.flat_param.data_ptr()
    assert opt.last_grad_norm.data_ptr() == opt.norm_dev.data_ptr() and opt.last_grad_norm.dim() == 0
    # the buffers are the optimizer's, allocated once: the second step reuses them and asks for no workspace size
    bucket.zero_grad()
    _set_grads(net)
    rec.calls.clear()
    opt.step(max_norm=0.5)
    assert [c[0] for c in rec.calls] == ["ign_gather_flat", "ign_grad_norm_clip", adam]
    assert _named(_lib, rec.calls[1], "ign_grad_norm_clip")["out2"] == norm["out2"]
    assert _named(_lib, rec.calls[1], "ign_grad_norm_clip")["workspace"] == norm["workspace"]


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("kw", [{}, {"max_norm": None}, {"max_norm": 0}])
def test_step_without_max_norm_calls_exactly_what_it_calls_today(host, capturable, kw):
    _lib, ddp, rec = host
    net = _net()
    bucket = ddp.FlatParamBucket(net, 1)
    opt = ddp.FlatAdam(bucket, lr=1e-3, capturable=capturable)
    _set_grads(net)
    rec.calls.clear()
    opt.step(**kw)
    adam = "ign_adam_step_dev" if capturable else "ign_adam_step"
    assert [c[0] for c in rec.calls] == ["ign_gather_flat", adam]
    step = _named(_lib, rec.calls[1], adam)
    assert step["grad"] == bucket.flat_grad.data_ptr() and step["n"] == bucket.flat_grad.numel() and step["stream"] == STREAM
    if not capturable:
        assert step["step"] == 1
    assert opt.norm_dev is None and opt.last_grad_norm is None


def test_accumulating_gather_names_the_acc_entry_point_and_keeps_the_bookkeeping(host):
    _lib, ddp, rec = host
    net = _net()
    ps = list(net.parameters())
    bucket = ddp.FlatParamBucket(net, 1)
    assert all(p.grad is None for p in ps)
    # first micro-step of a cycle: overwrite; parameter 3 has no gradient and a clean slot
    _set_grads(net, skip=(3,))
    g0 = [p.grad for p in ps]
    bucket.gather()
    assert [c[0] for c in rec.calls] == ["ign_gather_flat"]
    assert bucket._dirty == [True, True, True, False]
    bucket.zero_grad()
    # second micro-step: parameter 1 has no gradient -- it is not in the table, its slot is left alone and stays dirty
    _set_grads(net, skip=(1,))
    g1 = [p.grad for p in ps]
    rec.calls.clear()
    bucket.gather(accumulate=True)
    assert [c[0] for c in rec.calls] == ["ign_gather_flat_acc"]
    call = _named(_lib, rec.calls[0], "ign_gather_flat_acc")
    assert call["count"] == 3 and call["flat"] == bucket.flat_grad.data_ptr() and call["stream"] == STREAM
    assert call["src"] == [g1[0].data_ptr(), g1[2].data_ptr(), g1[3].data_ptr()]
    assert call["off"] == [bucket.offsets[0], bucket.offsets[2], bucket.offsets[3]]
    assert call["n"] == [15, 10, 2]
    assert all(p.grad is None for p in ps)
    assert bucket._dirty == [True, True, True, True]
    # the optimizer's own gather() closes the cycle: nothing is copied, nothing is zeroed, p.grad is the slot
    rec.calls.clear()
    before = bucket.flat_grad.clone()
    bucket.gather()
    assert rec.calls == [] and torch.equal(before, bucket.flat_grad)
    assert all(p.grad is v for p, v in zip(ps, bucket.views))
    assert bucket._dirty == [True, True, True, True]
    # next cycle, first micro-step: a parameter without a gradient has its dirty slot zero-filled again
    bucket.zero_grad()
    bucket.views[1].fill_(7.0)
    _set_grads(net, skip=(1,))
    rec.calls.clear()
    bucket.gather()
    assert [c[0] for c in rec.calls] == ["ign_gather_flat"]
    assert float(bucket.views[1].abs().max()) == 0.0 and bucket._dirty == [True, False, True, True]
    del g0


def test_clip_is_the_norm_launch_plus_one_scale_launch(host):
    _lib, ddp, rec = host
    net = _net()
    bucket = ddp.FlatParamBucket(net, 1)
    _set_grads(net)
    norm = bucket.clip_(2.0)
    assert [c[0] for c in rec.calls] == ["ign_gather_flat", "ign_grad_norm_workspace_bytes", "ign_grad_norm_clip", "ign_scale_flat"]
    out2 = _named(_lib, rec.calls[2], "ign_grad_norm_clip")["out2"]
    sc = _named(_lib, rec.calls[3], "ign_scale_flat")
    assert sc["g"] == bucket.flat_grad.data_ptr() and sc["n"] == bucket.flat_grad.numel() and sc["coef_dev"] == out2 + 4
    assert norm.dim() == 0 and norm.data_ptr() == out2


# ---------------------------------------------------------------- --hipgraph eligibility
def _experiment(**kw):
    import speech_imagery_eeg_amd  # noqa: F401
    from exp.experiment_classification import Experiment
    e = Experiment.__new__(Experiment)
    a = dict(hipgraph=True, gradient_accumulation_steps=2, gradient_clip=0.5, model="InterpGN", amp=False)
    a.update({k: v for k, v in kw.items() if k in a})
    e.args = Namespace(**a)
    e.device = torch.device(kw.get("device", "cuda"))
    e.distributed = kw.get("distributed", False)
    e.model = kw.get("module", torch.nn.Linear(2, 2))
    e._flat_step = kw.get("flat", True)
    return e


def test_graph_eligible_with_clipping_and_accumulation():
    assert _experiment()._graph_eligible(False) is True
    assert _experiment(gradient_accumulation_steps=1, gradient_clip=0.0)._graph_eligible(False) is True
    assert _experiment(model="SBM", gradient_accumulation_steps=4)._graph_eligible(False) is True


def test_graph_eligibility_keeps_its_other_conditions():
    from layers.SelfAttention_Family import FullAttention
    assert not _experiment()._graph_eligible(True)                         # amp
    assert not _experiment(distributed=True)._graph_eligible(False)
    assert not _experiment(model="DNN")._graph_eligible(False)
    assert not _experiment(model="EEGCNN")._graph_eligible(False)
    assert not _experiment(hipgraph=False)._graph_eligible(False)
    assert not _experiment(device="cpu")._graph_eligible(False)
    assert not _experiment(flat=False)._graph_eligible(False)             # another optimizer
    drop = torch.nn.Sequential(FullAttention(attention_dropout=0.1))
    assert not _experiment(module=drop)._graph_eligible(False)
    assert _experiment(module=torch.nn.Sequential(FullAttention(attention_dropout=0.0)))._graph_eligible(False)
