"""The explanation host path on the GPU (utils/explain.py): the four explainers -- input_saliency, evidence_map, faithfulness_curves,
occlusion_map -- leave a model exactly as they found it, and explain the class a plain eval forward predicts.  An InterpGN with the
FCN expert and an FCN alone at B=4, T=100, C=6, N=4 (the smallest shape at which every shapelet length group and the FCN's 14-sample
receptive field fit), each put in a mixed state first: train mode with one submodule in eval mode, one parameter that takes no
gradient, and the FCN's ``input_grad`` switch either an instance attribute or absent.  Every assertion is an identity; the host side
is tests/test_explain_host.py."""
import pytest
import torch

from conftest import make_cfg

pytestmark = pytest.mark.gpu
B_, T_, C_, N_ = 4, 100, 6, 4
SWITCHES = ("input_grad", "keep_last", "last_block")


def _setup(kind, switch_set):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import speech_imagery_eeg_amd  # noqa: F401
    from models.FullyConvNet import FullyConvNetwork
    from models.InterpGN import InterpGN
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = (InterpGN if kind == "InterpGN" else FullyConvNetwork)(make_cfg()).to(dev)
    fcn = model.deep_model if kind == "InterpGN" else model
    model.train()
    fcn.block2.eval()
    next(model.parameters()).requires_grad_(False)
    if switch_set:
        fcn.input_grad = False                                                          # an instance attribute that shadows the class's
    x = torch.randn(B_, T_, C_, generator=torch.Generator().manual_seed(1)).to(dev)
    return model, fcn, x


def _state(model, fcn):
    return ([m.training for m in model.modules()], [p.requires_grad for p in model.parameters()],
            {k: vars(fcn)[k] for k in SWITCHES if k in vars(fcn)})


def _plain_argmax(model, fcn, x, explain):
    """the arg-max of a plain eval forward of the explained logits, on a model that is put back into its mixed state"""
    from utils.explain import model_logits
    flags = [(m, m.training) for m in model.modules()]
    model.eval()
    with torch.no_grad():
        logits = {"sbm": lambda: model.sbm(x, None)[0], "gated": lambda: model(x, None, None, None, gating_value=None)[0],
                  "dnn": lambda: fcn(x), "model": lambda: model_logits(model, x)}[explain]()
    for m, flag in flags:
        m.training = flag
    return logits.argmax(1)


@pytest.mark.parametrize("switch_set", [True, False], ids=["switch-set", "switch-absent"])
@pytest.mark.parametrize("kind", ["InterpGN", "FCN"])
def test_explainers_restore_the_model_and_explain_the_predicted_class(kind, switch_set):
    model, fcn, x = _setup(kind, switch_set)
    from utils.evidence import evidence_map
    from utils.faithfulness import faithfulness_curves
    from utils.occlusion import occlusion_map
    from utils.saliency import input_saliency
    assert hasattr(fcn, "block2") and any(not m.training for m in model.modules()) and any(m.training for m in model.modules())
    before = _state(model, fcn)
    assert before[2] == ({"input_grad": False} if switch_set else {}) and not all(before[1]) and any(before[1])
    calls = 0
    for explain in (("sbm", "gated", "dnn", "model") if kind == "InterpGN" else ("dnn", "model")):
        want = _plain_argmax(model, fcn, x, explain)
        assert _state(model, fcn) == before
        reported = {}
        if explain != "model":
            assert input_saliency(model, x, explain=explain).shape == x.shape
            assert _state(model, fcn) == before and all(p.grad is None for p in model.parameters()), (explain, "saliency")
            reported["evidence"] = evidence_map(model, x, explain=explain).target
            assert _state(model, fcn) == before and all(p.grad is None for p in model.parameters()), (explain, "evidence")
        attributions = ("occlusion", "random") if explain == "model" else ("evidence", "saliency", "random")
        reported["faithfulness"] = faithfulness_curves(model, x, explain=explain, attributions=attributions, steps=2, window=50).target
        assert _state(model, fcn) == before and all(p.grad is None for p in model.parameters()), (explain, "faithfulness")
        reported["occlusion"] = occlusion_map(model, x, explain=explain, window=50, stride=25).target
        assert _state(model, fcn) == before and all(p.grad is None for p in model.parameters()), (explain, "occlusion")
        for name, target in reported.items():
            assert target.dtype == torch.long and torch.equal(target, want), (explain, name)
        calls += len(reported) + (explain != "model")
    assert calls == (14 if kind == "InterpGN" else 6)
