"""The explanation host path on the host (no GPU): utils/explain.py -- the dispatch of ``explain`` for every (model type, explain) pair
the four entry points accept or refuse, the session's restoration, the target rule, the lengths -- and the one loader loop of
Experiment.saliency / evidence / faithfulness / occlusion against recording stand-ins.  The GPU side is tests/test_gpu_explain.py."""
import os
import subprocess
import sys
from argparse import Namespace

import pytest
import torch

from conftest import ROOT, make_cfg

import speech_imagery_eeg_amd  # noqa: F401
from utils import explain as E

WHO = ("input_saliency", "evidence_map", "faithfulness_curves", "occlusion_map")


def _bare(cls):
    """an instance of a model class without its constructor's work (no kernels, no weights)"""
    m = cls.__new__(cls)
    torch.nn.Module.__init__(m)
    return m


def _models():
    from models.FullyConvNet import FullyConvNetwork
    from models.InterpGN import InterpGN
    from models.Shapelet import DistThresholdSBM, ShapeBottleneckModel
    from models.eegcnn import EEGCNNTransformer
    return dict(SBM=ShapeBottleneckModel(make_cfg()), LTS=DistThresholdSBM(make_cfg()), IGN=InterpGN(make_cfg()),
                IGN_ResNet=InterpGN(make_cfg(dnn_type="ResNet")), FCN=FullyConvNetwork(make_cfg()), EEGCNN=_bare(EEGCNNTransformer),
                Linear=torch.nn.Linear(2, 2))


# ---------------------------------------------------------------- the dispatch
def test_explained_gives_scope_sbm_fcn_for_every_accepted_pair():
    assert E.EXPLAIN == ("sbm", "gated", "dnn") and E.EXPLAIN_ALL == ("sbm", "gated", "dnn", "model")
    from utils import occlusion, saliency
    assert saliency.EXPLAIN == E.EXPLAIN and occlusion.EXPLAIN == ("model", "sbm", "gated", "dnn")
    m = _models()
    ign = m["IGN"]
    want = {("SBM", "sbm"): (m["SBM"], m["SBM"], None), ("LTS", "sbm"): (m["LTS"], m["LTS"], None),
            ("IGN", "sbm"): (ign.sbm, ign.sbm, None), ("IGN_ResNet", "sbm"): (m["IGN_ResNet"].sbm, m["IGN_ResNet"].sbm, None),
            ("IGN", "gated"): (ign, ign.sbm, ign.deep_model), ("IGN", "dnn"): (ign.deep_model, None, ign.deep_model),
            ("FCN", "dnn"): (m["FCN"], None, m["FCN"])}
    want.update({(name, "model"): (model, E.shapelet_expert(model), None) for name, model in m.items()})
    assert E.shapelet_expert(ign) is ign.sbm and E.shapelet_expert(m["LTS"]) is m["LTS"]
    assert all(E.shapelet_expert(m[name]) is None for name in ("FCN", "EEGCNN", "Linear"))
    for who in WHO:
        for (name, explain), (scope, sbm, fcn) in want.items():
            got = E.explained(m[name], explain, who)
            assert got.scope is scope and got.sbm is sbm and got.fcn is fcn and callable(got.call), (who, name, explain)
    refused = {(name, explain) for name in m for explain in E.EXPLAIN_ALL} - set(want)
    assert len(want) == 14 and len(refused) == 14                        # the other half is refused, below


def test_explained_refuses_every_other_pair_with_the_callers_name():
    m = _models()
    refused = {"sbm": (("FCN", "EEGCNN", "Linear"), "{who} explains a shapelet expert (SBM, LTS or the SBM inside InterpGN), not {cls}"),
               "gated": (("SBM", "LTS", "FCN", "EEGCNN", "Linear"), '{who}(explain="gated") needs an InterpGN with the FCN deep expert, not {cls}'),
               "dnn": (("SBM", "LTS", "EEGCNN", "Linear"),
                       '{who}(explain="dnn") needs an InterpGN or a FullyConvNetwork with the FCN deep expert, not {cls}')}
    count = 0
    for who in WHO:
        for explain, (names, text) in refused.items():
            for name in names:
                with pytest.raises(TypeError) as err:
                    E.explained(m[name], explain, who)
                assert str(err.value) == text.format(who=who, cls=type(m[name]).__name__)
                count += 1
        for explain in ("gated", "dnn"):
            with pytest.raises(TypeError) as err:
                E.explained(m["IGN_ResNet"], explain, who)
            assert str(err.value) == (f'{who}(explain="{explain}"): FCN is the supported deep expert (--dnn_type FCN), '
                                      f'not {type(m["IGN_ResNet"].deep_model).__name__}')
            count += 1
        with pytest.raises(TypeError) as err:
            E.explained(lambda v: v, "model", who)
        assert str(err.value) == f'{who}(explain="model") needs a torch.nn.Module, not function'
    assert count == 4 * 14


def test_call_follows_each_calling_convention():
    from models.InterpGN import InterpGN
    from models.Shapelet import ShapeBottleneckModel
    from models.eegcnn import EEGCNNTransformer
    seen = []
    x, mask = torch.zeros(2, 5, 3), torch.ones(2, 5)
    sbm = ShapeBottleneckModel(make_cfg())
    sbm.forward = lambda *a, **k: (seen.append(("sbm", a, k)) or (a[0].sum(1), "info"))
    assert E.explained(sbm, "sbm", "w").call(x, mask)[1] == "info" and seen[-1][1][1] is mask and seen[-1][2] == {}
    ign = InterpGN(make_cfg())
    ign.forward = lambda *a, **k: (seen.append(("ign", a, k)) or (a[0].sum(1), "info"))
    for explain in ("gated", "model"):
        logits, info = E.explained(ign, explain, "w", gating_value=0.25).call(x, mask)
        assert logits.shape == (2, 3) and info == ("info" if explain == "gated" else None)
        assert seen[-1][1][1:] == (mask, None, None) and seen[-1][2] == dict(gating_value=0.25)
    ign.deep_model.forward = lambda *a, **k: (seen.append(("fcn", a, k)) or a[0].sum(1))
    assert E.explained(ign, "dnn", "w").call(x, mask)[1] is None and seen[-1][1][0] is x and len(seen[-1][1]) == 1     # no mask reaches the FCN
    eeg = _bare(EEGCNNTransformer)
    eeg.forward = lambda v, *a, **k: (seen.append(("eeg", v.shape, a, k)) or (v.sum(2), None))
    logits, info = E.explained(eeg, "model", "w").call(x, mask)
    assert logits.shape == (2, 3) and info is None and seen[-1] == ("eeg", (2, 3, 5), (), {})                         # (B,C,T), no mask
    sbm2 = ShapeBottleneckModel(make_cfg())
    sbm2.forward = lambda *a, **k: (seen.append(("sbm2", a, k)) or (a[0].sum(1), "info"))
    assert E.explained(sbm2, "model", "w", gating_value=0.5).call(x, mask)[1] is None and seen[-1][1][1:] == (mask, None, None) and seen[-1][2] == {}


def test_require_linear_head():
    from models.Shapelet import ShapeBottleneckModel
    E.require_linear_head(None, "w")
    E.require_linear_head(ShapeBottleneckModel(make_cfg()), "w")
    for cls in ("bilinear", "attention"):
        with pytest.raises(ValueError, match=f"evidence_map: --sbm_cls {cls} is not additive"):
            E.require_linear_head(ShapeBottleneckModel(make_cfg(sbm_cls=cls)), "evidence_map")


# ---------------------------------------------------------------- the session
class _Fcn(torch.nn.Module):
    input_grad = False
    keep_last = False

    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(3, 2)


def _tree():
    """a module tree with mixed train / eval flags and mixed requires_grad flags"""
    fcn = _Fcn()
    tree = torch.nn.Sequential(torch.nn.Linear(3, 3), torch.nn.Sequential(torch.nn.BatchNorm1d(3), torch.nn.Dropout(0.5)), fcn)
    tree.train()
    tree[1][0].eval()
    fcn.eval()
    tree[0].bias.requires_grad_(False)
    fcn.fc.weight.requires_grad_(False)
    return tree, fcn


def _flags(tree):
    return [m.training for m in tree.modules()], [p.requires_grad for p in tree.parameters()]


def _leave(how, tree, **kw):
    """run a session to its end, out of it with an exception, or out of it with a return; -> what was seen inside"""
    def body():
        with E.session(tree, **kw):
            inside = dict(flags=_flags(tree), grad=torch.is_grad_enabled(), autocast=torch.is_autocast_enabled("cpu"),
                          switch={k: v for k, v in vars(kw["fcn"]).items() if k in ("input_grad", "keep_last")})
            if how == "return":
                return inside
            if how == "raise":
                raise KeyError(inside)
        return inside
    if how != "raise":
        return body()
    with pytest.raises(KeyError) as err:
        body()
    return err.value.args[0]


@pytest.mark.parametrize("how", ["exit", "raise", "return"])
def test_session_restores_flags_switches_and_contexts(how):
    tree, fcn = _tree()
    before = _flags(tree)
    assert True in before[0] and False in before[0] and True in before[1] and False in before[1]
    n = len(before[0])
    # no-grad session inside an ambient autocast with gradients on: eval, nothing frozen, no switch touched
    with torch.enable_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        inside = _leave(how, tree, fcn=fcn)
        assert inside == dict(flags=([False] * n, before[1]), grad=False, autocast=False, switch={})
        assert torch.is_grad_enabled() and torch.is_autocast_enabled("cpu")
    assert _flags(tree) == before and vars(fcn).keys() == vars(_Fcn()).keys()
    # grad session inside an ambient no_grad and autocast: gradients on, the autocast left as found, every parameter frozen
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        inside = _leave(how, tree, grad=True, freeze=True, fcn=fcn, switch="input_grad")
        assert inside == dict(flags=([False] * n, [False] * len(before[1])), grad=True, autocast=True, switch=dict(input_grad=True))
        assert not torch.is_grad_enabled() and torch.is_autocast_enabled("cpu")
    assert _flags(tree) == before and "input_grad" not in vars(fcn) and fcn.input_grad is False      # was no instance attribute: removed
    # the switch as an instance attribute comes back as it was; keep_last drops what the forward kept
    for switch, old in (("input_grad", False), ("input_grad", True), ("keep_last", False), ("keep_last", True)):
        setattr(fcn, switch, old)
        fcn.last_block = ("kept",)
        inside = _leave(how, tree, fcn=fcn, switch=switch)
        assert inside["switch"][switch] is True and inside["grad"] is False
        assert vars(fcn)[switch] is old and ("last_block" in vars(fcn)) == (switch != "keep_last")
        vars(fcn).pop(switch)
        vars(fcn).pop("last_block", None)
    inside = _leave(how, tree, fcn=fcn, switch="keep_last")
    assert inside["switch"] == dict(keep_last=True) and "keep_last" not in vars(fcn) and _flags(tree) == before
    assert not torch.is_autocast_enabled("cpu") and torch.is_grad_enabled()


# ---------------------------------------------------------------- the target rule, the lengths
def test_resolve_target_table():
    logits = torch.tensor([[0.0, 2.0, 1.0], [3.0, 0.0, 1.0], [0.0, 0.0, 5.0], [1.0, 4.0, 0.0]])
    R = E.resolve_target
    got = R(1, logits, "w")
    assert got.dtype == torch.long and got.tolist() == [1, 1, 1, 1]
    for dtype in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
        got = R(torch.tensor([2, 0, 1, 2], dtype=dtype), logits, "w")
        assert got.dtype == torch.long and got.shape == (4,) and got.tolist() == [2, 0, 1, 2]
    got = R(None, logits, "w")
    assert got.dtype == torch.long and got.tolist() == [1, 0, 2, 1]
    for bad in (torch.tensor([0, 1, 2]), torch.tensor([0, 1, 2, 0, 1]), torch.zeros(0, dtype=torch.long)):
        with pytest.raises(ValueError) as err:
            R(bad, logits, "evidence_map")
        assert str(err.value) == f"evidence_map: target has {bad.numel()} entries for a batch of 4"
    for bad in (-1, 3, torch.tensor([0, 1, 2, 3]), torch.tensor([0, -1, 2, 0])):
        with pytest.raises(ValueError) as err:
            R(bad, logits, "input_saliency")
        assert str(err.value) == "input_saliency: target outside [0, 3)"
    for target in (None, 2, torch.zeros(0, dtype=torch.int32)):
        got = R(target, logits[:0], "w")
        assert got.dtype == torch.long and got.shape == (0,)
    from utils import evidence
    assert evidence._resolve_target(None, logits).tolist() == [1, 0, 2, 1]
    with pytest.raises(ValueError, match=r"evidence_map: target outside \[0, 3\)"):
        evidence._resolve_target(7, logits)


def test_lengths_of_and_mean_fill():
    from models.Shapelet import ShapeBottleneckModel
    from utils import occlusion
    T = 12
    lengths = torch.tensor([12, 5, 0, 7])
    mask = (torch.arange(T)[None, :] < lengths[:, None]).float()
    on = ShapeBottleneckModel(make_cfg(enc_in=2, seq_len=T, num_class=3, mask_padding=True))
    off = ShapeBottleneckModel(make_cfg(enc_in=2, seq_len=T, num_class=3))
    assert E.lengths_of(None, mask, T) is None and E.lengths_of(off, mask, T) is None and E.lengths_of(on, None, T) is None
    got = E.lengths_of(on, mask, T)
    assert got.dtype == torch.int32 and got.tolist() == [12, 5, 0, 7] and got.is_contiguous()
    assert E.lengths_of(on, mask, 6).tolist() == [6, 5, 0, 6]                            # inside [0, T]
    assert occlusion.mean_fill is E.mean_fill and occlusion.model_logits is E.model_logits and occlusion.shapelet_expert is E.shapelet_expert
    x = torch.randn(4, T, 2, generator=torch.Generator().manual_seed(0))
    fill = E.mean_fill(x, got)
    assert torch.equal(E.mean_fill(x, None), x.mean(1)) and torch.allclose(fill[1], x[1, :5].mean(0)) and bool((fill[2] == 0).all())


def test_the_module_and_both_parsers_import_without_torch():
    code = ("import sys; sys.modules['torch'] = None; sys.path.insert(0, sys.argv[1]); import utils.explain as E; "
            "from utils.occlusion import parse_occlusion; from utils.faithfulness import parse_faithfulness; "
            "print(E.EXPLAIN_ALL[-1], parse_occlusion('explain=model,window=4').window, "
            "parse_faithfulness('explain=sbm,attr=evidence+random,steps=3').attributions, 'models' in sys.modules)")
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "speech-imagery-eeg_amd")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "model 4 ('evidence', 'random') False", out.stderr


# ---------------------------------------------------------------- the loader loop of the Experiment
T_, C_ = 7, 2


def _experiment(sizes):
    from exp.experiment_classification import Experiment
    gen = torch.Generator().manual_seed(3)
    batches = [(torch.randn(n, T_, C_, generator=gen), torch.zeros(n, dtype=torch.long), torch.ones(n, T_)) for n in sizes]
    exp = Experiment.__new__(Experiment)
    exp.model, exp.test_loader, exp.args = "the model", batches, Namespace(gating_value=0.5, seq_len=T_, enc_in=C_)
    exp._to_device = lambda x, y, m: (x + 0.0, y, m * 2.0)                              # "on the device": another tensor, a marked mask
    return exp, torch.cat([b[0] for b in batches])


def _stand_ins(monkeypatch, log):
    """the four explainers, recording what reaches them and answering with tensors that carry the batch"""
    from utils import evidence, faithfulness, occlusion, saliency

    def input_saliency(model, x, target=None, explain="sbm", gating_value=None):
        log.append(("saliency", model, x.shape[0], target, explain, gating_value, None))
        return 2.0 * x

    def evidence_map(model, x, target=None, explain="sbm", gating_value=None, mask=None):
        log.append(("evidence", model, x.shape[0], target, explain, gating_value, mask))
        return evidence.Evidence(sbm=x, logit=x[:, 0, 0], target=torch.arange(x.shape[0]))

    def faithfulness_curves(model, x, mask=None, target=None, seed=0, gating_value=None, **spec):
        log.append(("faithfulness", model, x.shape[0], target, spec, gating_value, mask, seed))
        f = faithfulness.Faithfulness(fractions=torch.tensor([0.0, 1.0]).double(), target=torch.arange(x.shape[0]), mode="deletion")
        f.logit["random"] = f.prob["random"] = x[:, :2, 0].t().contiguous()
        f.flip_at["random"] = x[:, 0, 1].double()
        return f

    def occlusion_map(model, x, mask=None, target=None, gating_value=None, **spec):
        log.append(("occlusion", model, x.shape[0], target, spec, gating_value, mask))
        return occlusion.Occlusion(map=x, drop=x[:, :, 0], target=torch.arange(x.shape[0]), base=x[:, 0, 0])

    monkeypatch.setattr(saliency, "input_saliency", input_saliency)
    monkeypatch.setattr(evidence, "evidence_map", evidence_map)
    monkeypatch.setattr(faithfulness, "faithfulness_curves", faithfulness_curves)
    monkeypatch.setattr(occlusion, "occlusion_map", occlusion_map)


def test_the_four_experiment_methods_walk_the_loader_once_in_order(monkeypatch):
    log = []
    _stand_ins(monkeypatch, log)
    exp, x = _experiment((3, 0, 2))
    sal = exp.saliency(target=1, explain="gated")
    assert torch.equal(sal, 2.0 * x) and sal.shape == (5, T_, C_)
    assert [e[2:] for e in log] == [(3, 1, "gated", None, None), (2, 1, "gated", None, None)]            # no --gating_value, no mask
    del log[:]
    ev = exp.evidence(explain="dnn")
    assert torch.equal(ev.sbm, x) and torch.equal(ev.logit, x[:, 0, 0]) and ev.target.tolist() == [0, 1, 2, 0, 1]
    assert ev.dnn is None and ev.cam is None and ev.eta is None and ev.remainder is None and ev.contrib is None
    assert [e[2:6] for e in log] == [(3, None, "dnn", 0.5), (2, None, "dnn", 0.5)] and all(bool((e[6] == 2.0).all()) for e in log)
    del log[:]
    f = exp.faithfulness(target=2, explain="sbm", steps=1, seed=40)
    assert torch.equal(f.logit["random"], x[:, :2, 0].t()) and torch.equal(f.flip_at["random"], x[:, 0, 1].double())
    assert f.target.tolist() == [0, 1, 2, 0, 1] and set(f.auc) == {"random"} and f.gap == {"random": 0.0}    # the summaries, recomputed
    assert [(e[2], e[3], e[4], e[5], e[7]) for e in log] == [(3, 2, dict(explain="sbm", steps=1), 0.5, 40), (2, 2, dict(explain="sbm", steps=1), 0.5, 41)]
    assert all(bool((e[6] == 2.0).all()) for e in log)                                   # seed + i counts the non-empty batches
    del log[:]
    occ = exp.occlusion(explain="model", window=3)
    assert torch.equal(occ.map, x) and torch.equal(occ.drop, x[:, :, 0]) and torch.equal(occ.base, x[:, 0, 0]) and occ.target.tolist() == [0, 1, 2, 0, 1]
    assert [e[2:6] for e in log] == [(3, None, dict(explain="model", window=3), 0.5), (2, None, dict(explain="model", window=3), 0.5)]
    assert all(e[1] == "the model" for e in log) and all(bool((e[6] == 2.0).all()) for e in log)
    assert not any(t.is_cuda for t in (sal, ev.sbm, f.target, occ.map))


def test_an_empty_loader_gives_the_empty_results(monkeypatch):
    import dataclasses
    log = []
    _stand_ins(monkeypatch, log)
    exp, _ = _experiment((0,))
    sal = exp.saliency()
    assert sal.shape == (0, T_, C_) and sal.dtype == torch.float32
    ev = exp.evidence()
    assert all(getattr(ev, f.name) is None for f in dataclasses.fields(ev))
    f = exp.faithfulness(explain="sbm")
    assert f.target is None and f.fractions is None and f.logit == f.prob == f.flip_at == f.auc == {}
    occ = exp.occlusion(explain="model")
    assert tuple(occ) == (None, None, None, None)
    assert log == []
    exp.test_loader = None
    assert exp.saliency(loader=[]).shape == (0, T_, C_) and exp.occlusion(loader=[], explain="model").map is None
