"""GPU parity of the gradient w.r.t. the INPUT series through the FCN expert and the gated mixture: the ign_clconv_dgrad_input*
kernels against float64, fcn_body(input_grad=True) against float64 torch modules, the InterpGN model against a fixture from the
reference's autograd (tests/golden/make_golden_fcn_input_grad.py) and utils.saliency.input_saliency(explain="gated" / "dnn")
against float64 autograd of the CPU oracle.  Gradient comparisons go through conftest.parity with kind="scale", tol=1e-4."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import golden, make_cfg, parity, sd_from

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _grad_close(label, got, ref, ref_is="oracle float64"):
    parity(label, got, ref, tol=1e-4, kind="scale", floor=1e-12, ref_is=ref_is)


def _bf16r(t):
    return t.float().bfloat16().double()


# ------------------------------------------------------------------------------------------------------------- the kernel
SHAPES = [(2, 40, 1, 16, 3), (2, 130, 6, 128, 8), (1, 257, 122, 128, 8), (2, 37, 3, 20, 2), (1, 64, 130, 128, 5), (3, 9, 5, 128, 3)]
GUARD = 1024


def _run_dgrad_input(dev, math, B, Tin, Ci, Co, k):
    """-> (gx (B,Tin,Ci) on the device, the guard region behind it, dy, w): one launch of the entry point of `math` into a
    NaN-filled buffer with GUARD sentinel floats after it."""
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(7 * Tin + Ci + Co + k)
    xs = 1e-6 if math.endswith("tiny") else 3e6 if math.endswith("huge") else 1.0
    math = math.split()[0]
    Tout, pad = Tin - k + 1, k - 1
    dy = torch.randn(B, Tout, Co, generator=g) * xs
    w = torch.randn(Co, Ci, k, generator=g) / (Co * k) ** 0.5 / xs ** 0.5
    dyp = F.pad(dy, (0, 0, pad, pad)).contiguous().to(dev)
    wdev = w.to(dev)
    n = B * Tin * Ci
    buf = torch.full((n + GUARD,), float("nan"), device=dev)
    buf[n:] = 12345.0
    gx = buf[:n].view(B, Tin, Ci)
    dims = (B, Tin, Ci, Co, k)
    if math == "f32":
        wt, wd = torch.empty(Co, k * Ci, device=dev), torch.empty(Ci, k * Co, device=dev)
        _lib.check(L.ign_clconv_pack_weights(_p(wdev), _p(wt), _p(wd), Co, Ci, k, _s()), "pack")
        _lib.check(L.ign_clconv_dgrad_input(_p(dyp), _p(wd), _p(gx), *dims, _s()), "dgrad_input")
    else:
        wt3 = torch.zeros(int(L.ign_clconv_x3_elems(Co, Ci, k)), device=dev, dtype=torch.bfloat16)
        wd3 = torch.zeros(int(L.ign_clconv_x3_elems(Ci, Co, k)), device=dev, dtype=torch.bfloat16)
        if math == "f16x3":
            # bounds: |W| exact, |dy| loose (4x): fp16's exponent range must not matter
            slots = torch.tensor([float(w.abs().max()), 0.0, 4.0 * float(dy.abs().max()), 0.0], device=dev)
            v1, i1 = ctypes.c_void_p * 1, ctypes.c_int * 1
            sp = lambda i: ctypes.c_void_p(slots.data_ptr() + 4 * i)
            _lib.check(L.ign_clconv_pack_weights_h2_multi(1, v1(wdev.data_ptr()), v1(wt3.data_ptr()), v1(wd3.data_ptr()), i1(Co), i1(Ci),
                                                          i1(k), None, v1(slots.data_ptr()), _s()), "pack_h2")
            _lib.check(L.ign_clconv_dgrad_input_h3(_p(dyp), _p(wd3), _p(gx), sp(2), sp(0), *dims, _s()), "dgrad_input_h3")
        else:
            _lib.check(L.ign_clconv_pack_weights_x3(_p(wdev), _p(wt3), _p(wd3), Co, Ci, k, _s()), "pack_x3")
            fn = L.ign_clconv_dgrad_input_x6 if math == "bf16x6" else L.ign_clconv_dgrad_input_bf16
            _lib.check(fn(_p(dyp), _p(wd3), _p(gx), *dims, _s()), "dgrad_input_" + math)
    torch.cuda.synchronize()
    return gx, buf[n:], dy, w


@pytest.mark.parametrize("B,Tin,Ci,Co,k", SHAPES)
@pytest.mark.parametrize("math", ["f32", "bf16x6", "f16x3", "f16x3 tiny", "f16x3 huge", "bf16"])
def test_clconv_dgrad_input_matches_conv_transpose1d(B, Tin, Ci, Co, k, math):
    """gx[b,t,ci] = sum_{jj,co} dyp[b,t+jj,co] W[co,ci,k-1-jj] == conv_transpose1d(dy, W) in float64, at fp32 rounding level (the
    bound test_gpu_fcn.py uses for the sibling GEMMs); "bf16": the float64 result of the bf16-ROUNDED operands.  Every element of
    gx is written and nothing behind it."""
    dev = _dev()
    gx, guard, dy, w = _run_dgrad_input(dev, math, B, Tin, Ci, Co, k)
    if math == "bf16":
        ref = F.conv_transpose1d(_bf16r(dy).permute(0, 2, 1), _bf16r(w)).permute(0, 2, 1)
    else:
        ref = F.conv_transpose1d(dy.double().permute(0, 2, 1), w.double()).permute(0, 2, 1)
    assert ref.shape == (B, Tin, Ci)
    assert bool(torch.isfinite(gx).all()), "an element of gx was left unwritten"
    assert bool((guard == 12345.0).all()), "a store went past gx"
    err = _rel(gx, ref)
    print(f"dgrad_input {math} {(B, Tin, Ci, Co, k)}: rel err {err:.3e}")
    assert err < 3e-6


@pytest.mark.parametrize("math", ["f32", "bf16x6", "f16x3"])
def test_clconv_dgrad_input_is_bitwise_repeatable(math):
    dev = _dev()
    a = _run_dgrad_input(dev, math, 1, 257, 122, 128, 8)[0].clone()
    b = _run_dgrad_input(dev, math, 1, 257, 122, 128, 8)[0].clone()
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ fcn_body against float64 modules
class _RefNet(nn.Module):
    """Conv1d + BatchNorm1d + ReLU x3, mean pool, Linear (IGN/model/FullyConvNet.py:31-59) keeping the pre-activations."""

    def __init__(self, C, N):
        super().__init__()
        ci, blocks = C, []
        for co, k in zip((128, 256, 128), (8, 5, 3)):
            blocks.append(nn.Sequential(nn.Conv1d(ci, co, k), nn.BatchNorm1d(co), nn.ReLU()))
            ci = co
        self.blocks = nn.Sequential(*blocks)
        self.fc = nn.Linear(128, N)
        with torch.no_grad():
            for b in self.blocks:                # non-trivial affine / running state
                b[1].weight.uniform_(0.5, 1.5)
                b[1].bias.normal_(0, 0.3)
                b[1].running_mean.normal_(0, 0.2)
                b[1].running_var.uniform_(0.5, 2.0)

    def forward(self, x_btc):
        h, pre = x_btc.permute(0, 2, 1), []
        for b in self.blocks:
            n = b[1](b[0](h))
            pre.append(n)
            h = b[2](n)
        pooled = h.mean(-1)
        return pooled, self.fc(pooled), pre


_BODY_REF = {}
BODY_SEEDS = {(4, 50, 6, True): 2, (4, 50, 6, False): 3, (2, 140, 122, True): 1, (2, 140, 122, False): 2}     # the condition below holds


def _body_reference(B, T, C, training):
    """float64 reference of one (shape, mode), computed once and shared: inputs, module, and per head / no head the outputs and
    gradients.  Asserts the condition on the inputs: float32 and float64 torch modules produce identical ReLU masks in all three
    blocks (the gradient is discontinuous at the kink), and no float64 pre-activation is within 1e-5 of it."""
    key = (B, T, C, training)
    if key in _BODY_REF:
        return _BODY_REF[key]
    seed = BODY_SEEDS[key]
    torch.manual_seed(seed)
    net32 = _RefNet(C, 4).train(training)
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(B, T, C, generator=g)
    gp, gl = torch.randn(B, 128, generator=g), torch.randn(B, 4, generator=g)
    net64 = copy.deepcopy(net32).double()
    with torch.no_grad():
        pre32 = copy.deepcopy(net32)(x)[2]       # (copies: a train-mode forward moves the running statistics)
        pre64 = copy.deepcopy(net64)(x.double())[2]
    for l, (a, b) in enumerate(zip(pre32, pre64)):
        assert torch.equal(a > 0, b > 0), f"block {l + 1}: float32 and float64 disagree on a ReLU mask (pick another seed)"
        assert int((b.abs() < 1e-5).sum()) == 0, f"block {l + 1}: a pre-activation sits on the ReLU kink (pick another seed)"
    res = {}
    for head in (False, True):
        n64 = copy.deepcopy(net64)
        x64 = x.double().requires_grad_(True)
        pooled, logits, _ = n64(x64)
        ((logits * gl.double()).sum() if head else (pooled * gp.double()).sum()).backward()
        res[head] = dict(out=(logits if head else pooled).detach(), gx=x64.grad, params={n: p.grad for n, p in n64.named_parameters()},
                         buffers={n: b.detach().clone() for n, b in n64.named_buffers()})
    _BODY_REF[key] = (net32, x, gp, gl, res)
    return _BODY_REF[key]


@pytest.mark.parametrize("B,T,C", [(4, 50, 6), (2, 140, 122)])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("head", [False, True], ids=["pooled", "fused-head"])
@pytest.mark.parametrize("math", ["f32", "bf16x6", "f16x3"])
def test_fcn_body_input_grad(B, T, C, training, head, math, monkeypatch):
    net32, x, gp, gl, res = _body_reference(B, T, C, training)        # (CPU conditions first)
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import fcn
    monkeypatch.setattr(fcn, "CONV_MATH", math)
    ref = res[head]
    mod = copy.deepcopy(net32).to(dev).train(training)
    blocks = [(b[0], b[1]) for b in mod.blocks]
    xd = x.to(dev).requires_grad_(True)
    out = fcn.fcn_body(xd, blocks, head=mod.fc if head else None, input_grad=True)
    (out * (gl if head else gp).to(dev)).sum().backward()
    assert _rel(out, ref["out"]) < TOL
    assert xd.grad is not None and xd.grad.shape == x.shape
    _grad_close(f"fcn_body x.grad {math} train={training} head={head} {(B, T, C)}", xd.grad, ref["gx"], ref_is="torch modules float64")
    for n, p in mod.named_parameters():
        q = ref["params"][n]
        if n.startswith("fc.") and not head:
            assert p.grad is None
            continue
        if training and n.endswith("0.bias"):
            # true gradient is zero (batch statistics remove the bias); both sides hold at most rounding noise
            assert float(p.grad.abs().max()) <= 1e-4 * max(1.0, float(q.abs().max())), n
            continue
        assert _rel(p.grad, q) < 2 * TOL, n
    for n, b in mod.named_buffers():
        if b.dtype.is_floating_point:
            assert _rel(b, ref["buffers"][n]) < TOL, n


# ------------------------------------------------------------------------------------------------------------ the fixture
def _ign_from_fixture(g, dev):
    import speech_imagery_eeg_amd  # noqa
    from models.InterpGN import InterpGN
    x = torch.from_numpy(g["x"])
    B, T, C = x.shape
    N = g["eval.out"].shape[1]
    m = InterpGN(make_cfg(enc_in=C, seq_len=T, num_class=N, c_out=N, dec_in=C))
    m.load_state_dict(sd_from(g))
    return m.to(dev), x


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_interpgn_input_grad_matches_the_reference(mode):
    dev = _dev()
    g = golden("ign_fcn_input_grad")
    m, x = _ign_from_fixture(g, dev)
    m.deep_model.input_grad = True
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for what in ("out", "dnn_preds"):
        m.load_state_dict(sd)                                           # (a train-mode forward moves the running statistics)
        m.train(mode == "train")
        xd = x.to(dev).requires_grad_(True)
        out, info = m(xd)
        if what == "out":
            parity(f"{mode} out", out, g[f"{mode}.out"], tol=1e-4, kind="elem")
            parity(f"{mode} eta", info.eta, g[f"{mode}.eta"], tol=1e-4, kind="elem")
            parity(f"{mode} dnn_preds", info.dnn_preds, g[f"{mode}.dnn_preds"], tol=1e-4, kind="elem")
            out.sum().backward()
            _grad_close(f"{mode} grad_x", xd.grad, g[f"{mode}.grad_x"], ref_is="reference fp32")
        else:
            info.dnn_preds.sum().backward()
            _grad_close(f"{mode} grad_x_dnn", xd.grad, g[f"{mode}.grad_x_dnn"], ref_is="reference fp32")


# --------------------------------------------------------------------------------------------------------------- saliency
def _assert_no_l1_ties(xn, ws):
    """no sample of the normalised series is bit-equal to a shapelet weight of its channel (there the kernel's documented
    sign(0) = -1 differs from aten::sgn)"""
    x = xn.detach().cpu().numpy()
    for w in ws:
        wn = w.detach().cpu().numpy()
        for c in range(x.shape[1]):
            assert np.intersect1d(x[:, c, :].ravel(), wn[:, c, :].ravel()).size == 0, f"exact tie in channel {c}"


def _saliency_model(dev, dnn_type="FCN"):
    import speech_imagery_eeg_amd  # noqa
    from models.InterpGN import InterpGN
    torch.manual_seed(6)
    cfg = make_cfg(enc_in=5, seq_len=80, num_class=4, c_out=4, dec_in=5, dnn_type=dnn_type)
    m = InterpGN(cfg).to(dev).train()
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for _ in range(3):                                             # non-trivial running statistics
            m(torch.randn(8, 80, 5, generator=gen).to(dev) * 1.5 + 0.2)
    x = torch.randn(4, 80, 5, generator=gen).to(dev)
    return m, x


def _oracle_ign(m):
    from oracle import ign_oracle as O
    ref = O.OracleIGN(m.configs, chunk=64)
    ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    return ref.double().eval()


def _oracle_grad(ref, x, idx, explain, gating_value=None):
    x64 = x.detach().cpu().double().requires_grad_(True)
    out, info = ref(x64, gating_value=gating_value)
    logits = out if explain == "gated" else info.dnn_preds
    logits.gather(1, idx.cpu()[:, None]).sum().backward()
    return logits.detach(), x64.grad


def test_input_saliency_gated_and_dnn():
    dev = _dev()
    m, x = _saliency_model(dev)
    from ign_hip import _lib
    from oracle import ign_oracle as O
    from utils.saliency import input_saliency
    _assert_no_l1_ties(O.instance_norm(x.cpu()), [s.weights for s in m.sbm.shapelets])
    B = x.shape[0]
    required = [p.requires_grad for p in m.parameters()]
    m.sbm.dropout.eval()                                              # a mixed train / eval set-up must come back as it was
    modes = [mod.training for mod in m.modules()]
    ref = _oracle_ign(m)

    _lib.timing_enable(True)
    sal = input_saliency(m, x, explain="gated")                       # predicted class of the MIXTURE
    counts = {k: _lib.timing_read(k)[1] for k in ("clconv_wgrad", "clconv_dgrad_input", "clconv_dgrad", "shp_bwd", "shp_bwd_x")}
    _lib.timing_enable(False)
    assert counts["clconv_wgrad"] == 0 and counts["shp_bwd"] == 0, "saliency must not run the weight-gradient launches"
    assert counts["clconv_dgrad_input"] == 1 and counts["clconv_dgrad"] == 2 and counts["shp_bwd_x"] == len(m.sbm.shapelets)
    assert sal.shape == x.shape and sal.device == x.device and bool(torch.isfinite(sal).all())

    def restored():
        assert all(p.grad is None for p in m.parameters())
        assert [p.requires_grad for p in m.parameters()] == required and m.training and not x.requires_grad
        assert [mod.training for mod in m.modules()] == modes and not m.sbm.dropout.training
        assert m.deep_model.input_grad is False and "input_grad" not in vars(m.deep_model)
    restored()

    with torch.no_grad():
        m.eval()
        out, info = m(x)
        m.train()
        m.sbm.dropout.eval()
    for explain, logits in (("gated", out), ("dnn", info.dnn_preds)):
        pred = logits.argmax(dim=1)
        out0, g0 = _oracle_grad(ref, x, pred, explain)
        parity(f"{explain} logits", logits, out0, tol=1e-4, kind="elem", ref_is="oracle float64")
        got = sal if explain == "gated" else input_saliency(m, x, explain=explain)
        _grad_close(f"saliency {explain}(pred)", got, g0)
        assert torch.equal(input_saliency(m, x, pred, explain=explain), got)         # a (B,) tensor
        tgt = torch.full((B,), 2, dtype=torch.long)
        _grad_close(f"saliency {explain}(2)", input_saliency(m, x, 2, explain=explain), _oracle_grad(ref, x, tgt, explain)[1])
        with pytest.raises(ValueError):
            input_saliency(m, x, 4, explain=explain)                   # out of range: raises inside the call ...
        restored()                                                     # ... and every flag is back
    # the default is the interpretable expert, bit for bit
    sbm = input_saliency(m, x, 1)
    assert torch.equal(input_saliency(m, x, 1, explain="sbm"), sbm)
    # gating_value = -1: every eta snaps to 1, the FCN contributes exactly zero and the mixture IS the SBM
    _grad_close("saliency gated, eta snapped to 1", input_saliency(m, x, 1, explain="gated", gating_value=-1.0), sbm,
                ref_is="input_saliency(explain='sbm')")
    tgt = torch.full((B,), 1, dtype=torch.long)
    _grad_close("saliency gated, eta snapped to 1 (oracle)", input_saliency(m, x, 1, explain="gated", gating_value=-1.0),
                _oracle_grad(ref, x, tgt, "gated", gating_value=-1.0)[1])
    assert torch.equal(input_saliency(m, x, 1, explain="dnn", gating_value=-1.0), input_saliency(m, x, 1, explain="dnn"))
    # a bare FCN expert is accepted with explain="dnn"
    assert torch.equal(input_saliency(m.deep_model, x, 1, explain="dnn"), input_saliency(m, x, 1, explain="dnn"))
    restored()


def test_input_gradient_stays_off_by_default():
    dev = _dev()
    m, x = _saliency_model(dev)
    from ign_hip import _lib
    from utils.saliency import input_saliency
    assert m.deep_model.input_grad is False
    xd = x.clone().requires_grad_(True)
    with pytest.raises(_lib.IgnError, match="input series"):
        m(xd)[0].sum().backward()
    import speech_imagery_eeg_amd  # noqa
    from models.InterpGN import InterpGN
    other = InterpGN(make_cfg(enc_in=5, seq_len=80, num_class=4, c_out=4, dec_in=5, dnn_type="ResNet")).to(dev)
    for explain in ("gated", "dnn"):
        with pytest.raises((TypeError, _lib.IgnError), match="FCN"):
            input_saliency(other, x, explain=explain)
    assert other.training and all(p.requires_grad for p in other.parameters())


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_parameter_grads_do_not_depend_on_the_input_gradient(training):
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from models.InterpGN import InterpGN
    torch.manual_seed(4)
    m = InterpGN(make_cfg(enc_in=5, seq_len=80, num_class=3, c_out=3, dec_in=5)).to(dev).train(training)
    x = torch.randn(6, 80, 5, generator=torch.Generator().manual_seed(5)).to(dev)
    y = (torch.arange(6) % 3).to(dev)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    grads = []
    for need_x, switch in ((False, False), (True, True), (False, True)):
        m.load_state_dict(sd)
        m.zero_grad(set_to_none=True)
        m.deep_model.input_grad = switch
        xd = x.clone().requires_grad_(need_x)
        out, info = m(xd)
        (F.cross_entropy(out, y) + info.loss.mean()).backward()
        assert (xd.grad is not None) == need_x
        grads.append({n: p.grad.clone() for n, p in m.named_parameters()})
    for other in grads[1:]:
        assert set(other) == set(grads[0])
        for n in grads[0]:
            assert torch.equal(grads[0][n], other[n]), n


def test_two_expert_streams_give_the_one_stream_saliency():
    """B*T*C just over InterpGN.two_stream_min_elems: the FCN expert runs on the side stream and the two experts' input gradients
    meet in autograd's accumulation across streams.  A sum of two terms is commutative: the result is bitwise the one-stream one."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from models.InterpGN import InterpGN
    from utils.saliency import input_saliency
    torch.manual_seed(9)
    m = InterpGN(make_cfg(enc_in=122, seq_len=1000, num_class=3, c_out=3, dec_in=122)).to(dev).eval()
    x = torch.randn(18, 1000, 122, generator=torch.Generator().manual_seed(10)).to(dev)
    assert x.numel() >= InterpGN.two_stream_min_elems
    was = InterpGN.expert_streams
    try:
        InterpGN.expert_streams = True
        two = input_saliency(m, x, 1, explain="gated")
        InterpGN.expert_streams = False
        one = input_saliency(m, x, 1, explain="gated")
    finally:
        InterpGN.expert_streams = was
    assert bool(torch.isfinite(one).all()) and float(one.abs().max()) > 0.0
    assert torch.equal(two, one)


def test_experiment_saliency_passes_explain_through():
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from argparse import Namespace
    from exp.experiment_classification import Experiment
    from models.InterpGN import InterpGN
    from utils.saliency import input_saliency
    torch.manual_seed(8)
    cfg = make_cfg(enc_in=3, seq_len=40, num_class=2, c_out=2, dec_in=3)
    exp = Experiment.__new__(Experiment)
    exp.model, exp.device, exp.args = InterpGN(cfg).to(dev), dev, Namespace(seq_len=40, enc_in=3)
    batches = [(torch.randn(n, 40, 3), torch.zeros(n), torch.ones(n, 40)) for n in (3, 2)]
    exp.test_loader = batches
    sal = exp.saliency(target=1, explain="gated")
    assert sal.shape == (5, 40, 3) and sal.device.type == "cpu"
    assert torch.equal(sal[:3], input_saliency(exp.model, batches[0][0].to(dev), 1, explain="gated").cpu())
    assert torch.equal(sal[3:], input_saliency(exp.model, batches[1][0].to(dev), 1, explain="gated").cpu())
    assert not torch.equal(sal, exp.saliency(target=1))                # the default still explains the SBM alone
    assert exp.saliency(loader=batches[:1], explain="dnn").shape == (3, 40, 3)
