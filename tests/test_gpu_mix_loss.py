"""The soft-label loss tail (ign_loss_mix_fwd_bwd_reg behind ops.ign_loss(..., y_b=, lam=)) on the GPU: against float64 (gini gate +
the criterion CEm of utils/mix.py written out in torch float64 + autograd on the CPU), its reductions to the hard-label tail, the
symmetry of the two labels, the scale invariance of the weights, bitwise repeatability, the gate left as it is, and one model step
against the torch composition utils.mix.mix_cross_entropy.

Bounds and kinds are those tests/test_gpu_class_weight.py uses for ign_loss_w_fwd_bwd_reg: 1e-5 "elem" for the loss, out and eta,
1e-5 "scale" for gsbm and gdnn.  Logits are randn * 3, the weights lie in [0.2, 5] with class 0 at 50 times the largest of the
others, the last class never occurs as a first label, lam is uniform with exact 0 and 1 among its values.

The caveat of that file holds here too.  A batch of ONE row: gdnn = (1 - eta) * go, and that row alone sets the scale gdnn is judged
against.  The fp32 gate rule (kept bitwise ign_gate_fwd's up to 16 classes) carries an absolute error in eta of the order of 1e-7
(that file: about 2.4e-7 at N = 2; observed here 1.4e-7 at N = 2 and 3.7e-8 .. 7.0e-8 at N = 16 .. 256, the wave-per-row layout
included), so 1e-5 of scale can be asked of a single row only while 1 - eta >= 0.024: the single row is drawn again (same generator)
until its float64 1 - eta is at least 0.1, at every N.  Larger batches have rows of every eta and need no such rule.

IGN_MIX_RECORD=<file> keeps every observed error (profiles/mix.json holds one such run)."""
import json
import os

import pytest
import torch
from conftest import make_cfg, parity

pytestmark = pytest.mark.gpu
REG = 0.125
# N: 2 smallest, 3 a narrow row, 16 | 17 the last thread-per-row and the first wave-per-row width, 39 CHISCO, 256 every chunk full
# B: 1, 5, 257 (thread 0 takes a second row / the 16 waves wrap), 300
NS, BS = [2, 3, 16, 17, 39, 256], [1, 5, 257, 300]
# (class weights, label smoothing, reg given, beta): every value of every option, with and without each other
OPTIONS = [(True, 0.1, True, 0.7), (False, 0.0, False, 0.0), (True, 0.0, False, 0.7), (False, 0.1, True, 0.0)]
_SEEN = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import speech_imagery_eeg_amd  # noqa: F401
    return torch.device("cuda:0")


def _case(B, N):
    """-> host tensors (s, d, ya, yb, lam, w); the single row of B == 1 by the rule of the module docstring"""
    g = torch.Generator().manual_seed(1000 * N + B)
    while True:
        s, d = torch.randn(B, N, generator=g) * 3, torch.randn(B, N, generator=g) * 3
        q = torch.softmax(s.double(), -1)
        if B > 1 or float(1 - ((q * q).sum() * N - 1) / (N - 1)) >= 0.1:
            break
    ya = torch.randint(0, N - 1, (B,), generator=g)
    ya[0] = 0
    yb = torch.randint(0, N, (B,), generator=g)
    lam = torch.rand(B, generator=g)
    if B > 2:
        lam[1], lam[2] = 0.0, 1.0
    w = 0.2 + 4.8 * torch.rand(N, generator=g)
    w[0] = 50.0 * w[1:].max()
    return s, d, ya, yb, lam, w


def _cem64(z, ya, yb, lam, w, eps):
    """CEm of utils/mix.py in differentiable float64 torch"""
    B, N = z.shape
    lp = torch.log_softmax(z, -1)
    w = torch.ones(N, dtype=torch.float64) if w is None else w.double()
    lam = lam.double()
    a, c = lam * w[ya], (1 - lam) * w[yb]
    rows = torch.arange(B)
    return ((1 - eps) * (a * -lp[rows, ya] + c * -lp[rows, yb]).sum() + (eps / N) * (-lp * w).sum()) / (a + c).sum()


def _oracle(s, d, ya, yb, lam, w, eps, reg, beta):
    s = s.double().requires_grad_(True)
    d = d.double().requires_grad_(True)
    N = s.shape[1]
    q = torch.softmax(s, -1)
    eta = ((q * q).sum(-1, keepdim=True) * N - 1) / (N - 1)
    out = eta * s + (1 - eta) * d
    loss = _cem64(out, ya, yb, lam, w, eps) + beta * _cem64(s, ya, yb, lam, w, eps) + (REG if reg else 0.0)
    loss.backward()
    return loss.detach(), out.detach(), eta.detach(), s.grad, d.grad


def _run(dev, s, d, ya, yb, lam, w, eps, reg, beta, soft=True):
    from ign_hip import ops
    sv, dv = s.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    kw = dict(reg=torch.tensor([REG], device=dev) if reg else None, class_weight=None if w is None else w.to(dev), label_smoothing=eps)
    if soft:
        kw.update(y_b=yb.to(dev), lam=lam.to(dev))
    loss, out, eta = ops.ign_loss(sv, dv, ya.to(dev), beta, **kw)
    loss.backward()
    return loss.detach(), out, eta, sv.grad, dv.grad


def _compare(tag, got, want, ref_is):
    for name, kind, g, r in zip(("loss", "out", "eta", "gsbm", "gdnn"), ("elem", "elem", "elem", "scale", "scale"), got, want):
        if name == "eta":
            r = r.reshape(g.shape)
        _SEEN[f"{tag}.{name}"] = parity(f"{tag}.{name}", g, r, tol=1e-5, kind=kind, ref_is=ref_is)


@pytest.fixture(scope="module", autouse=True)
def _write_seen():
    yield
    path = os.environ.get("IGN_MIX_RECORD")
    if _SEEN and path:
        keep = ("max_abs_err", "scale", "kind", "tol", "against")
        worst = max(_SEEN.items(), key=lambda kv: kv[1]["err_over_1e4"])
        with open(path, "w") as f:
            json.dump(dict(bound="1e-5: elem for loss / out / eta, of scale for gsbm / gdnn", worst=dict(tensor=worst[0], **worst[1]),
                           records={k: {q: v[q] for q in keep} | {"err_over_tol": v["err_over_1e4"] * 1e-4 / v["tol"]}
                                    for k, v in sorted(_SEEN.items())}), f, indent=1, sort_keys=True)


# ---------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("weights,eps,reg,beta", OPTIONS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("N", NS)
def test_soft_label_tail_vs_float64(N, B, weights, eps, reg, beta):
    dev = _dev()
    s, d, ya, yb, lam, w = _case(B, N)
    w = w if weights else None
    want = _oracle(s, d, ya, yb, lam, w, eps, reg, beta)
    got = _run(dev, s, d, ya, yb, lam, w, eps, reg, beta)
    _compare(f"mix_n{N}_b{B}_w{int(weights)}_e{eps}_r{int(reg)}_beta{beta}", got, want, "float64")


# ---------------------------------------------------------------- 2. reductions to the hard-label tail
@pytest.mark.parametrize("weights,eps", [(True, 0.1), (False, 0.0)])
@pytest.mark.parametrize("B,N", [(5, 3), (257, 16), (300, 17), (257, 256)])
def test_lam_one_is_the_hard_label_call(B, N, weights, eps):
    dev = _dev()
    s, d, ya, yb, lam, w = _case(B, N)
    w = w if weights else None
    hard = _run(dev, s, d, ya, yb, lam, w, eps, True, 0.7, soft=False)
    got = _run(dev, s, d, ya, yb, torch.ones(B), w, eps, True, 0.7)
    _compare(f"mix_lam1_n{N}_b{B}_w{int(weights)}", got, hard, "ops.ign_loss without soft labels")


@pytest.mark.parametrize("B,N", [(5, 3), (257, 16), (300, 17), (257, 256)])
def test_equal_labels_are_the_hard_label_call_at_any_lam(B, N):
    dev = _dev()
    s, d, ya, yb, lam, w = _case(B, N)
    hard = _run(dev, s, d, ya, yb, lam, w, 0.1, True, 0.7, soft=False)
    got = _run(dev, s, d, ya, ya, lam, w, 0.1, True, 0.7)
    _compare(f"mix_same_n{N}_b{B}", got, hard, "ops.ign_loss without soft labels")


# ---------------------------------------------------------------- 3. symmetry and scaling
@pytest.mark.parametrize("B,N", [(257, 16), (300, 39)])
def test_swapping_the_two_labels(B, N):
    dev = _dev()
    s, d, ya, yb, lam, w = _case(B, N)
    a = _run(dev, s, d, ya, yb, lam, w, 0.1, True, 0.7)
    b = _run(dev, s, d, yb, ya, 1 - lam, w, 0.1, True, 0.7)
    _compare(f"mix_swap_n{N}", b, a, "the same call with (ya, lam) and (yb, 1 - lam) swapped")


@pytest.mark.parametrize("B,N", [(257, 16), (300, 39)])
def test_scale_invariance(B, N):
    dev = _dev()
    s, d, ya, yb, lam, w = _case(B, N)
    a, b = _run(dev, s, d, ya, yb, lam, w, 0.1, True, 0.7), _run(dev, s, d, ya, yb, lam, w / 4, 0.1, True, 0.7)
    _compare(f"mix_scale_n{N}", b, a, "the same call with 4 w")


# ---------------------------------------------------------------- 4. repeatability and the gate
@pytest.mark.parametrize("B,N", [(257, 16), (300, 39)])
def test_two_calls_are_bitwise_equal(B, N):
    dev = _dev()
    s, d, ya, yb, lam, w = _case(B, N)
    a, b = _run(dev, s, d, ya, yb, lam, w, 0.1, True, 0.7), _run(dev, s, d, ya, yb, lam, w, 0.1, True, 0.7)
    for name, u, v in zip(("loss", "out", "eta", "gsbm", "gdnn"), a, b):
        assert torch.equal(u, v), name


@pytest.mark.parametrize("B,N", [(1, 2), (5, 3), (257, 16)])
def test_gate_is_unchanged_up_to_16_classes(B, N):
    dev = _dev()
    from ign_hip import ops
    s, d, ya, yb, lam, w = _case(B, N)
    _, out, eta, _, _ = _run(dev, s, d, ya, yb, lam, w, 0.1, True, 0.7)
    out_g, eta_g = ops.gini_gate(s.to(dev), d.to(dev))
    assert torch.equal(out, out_g) and torch.equal(eta, eta_g)


def test_labels_and_lam_out_of_range_are_clamped():
    dev = _dev()
    B, N = 5, 3
    s, d, ya, yb, lam, w = _case(B, N)
    ya2, yb2, lam2 = ya.clone(), yb.clone(), lam.clone()
    ya2[3], yb2[4], lam2[0], lam2[3] = 7, -2, 1.5, -0.25
    got = _run(dev, s, d, ya2, yb2, lam2, w, 0.1, True, 0.7)
    ya2[3], yb2[4], lam2[0], lam2[3] = N - 1, 0, 1.0, 0.0
    want = _run(dev, s, d, ya2, yb2, lam2, w, 0.1, True, 0.7)
    for name, u, v in zip(("loss", "out", "eta", "gsbm", "gdnn"), got, want):
        assert torch.equal(u, v), name


# ---------------------------------------------------------------- 5. one model step
def test_model_step_equals_the_torch_composition():
    """A tiny InterpGN (FCN expert): one backward pass under the fused soft-label tail, one under the loss composed from
    utils.mix.mix_cross_entropy on the model's own GPU logits.  Only the tail differs, so the loss and the parameter gradients agree
    to 1e-5 of each one's scale."""
    dev = _dev()
    from ign_hip import ops
    from models.InterpGN import InterpGN
    from utils.mix import mix_cross_entropy
    B, T, C, N, eps, beta = 6, 40, 3, 4, 0.1, 0.37
    torch.manual_seed(0)
    m = InterpGN(make_cfg(enc_in=C, seq_len=T, num_class=N, c_out=N, dec_in=C)).to(dev).train()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, T, C, generator=g).to(dev)
    ya = torch.tensor([0, 1, 2, 0, 1, 0], device=dev)              # class 3 occurs only as a second label
    yb = ya.roll(-1).clone()
    yb[5] = 3
    lam = torch.tensor([0.3, 1.0, 0.0, 0.85, 0.5, 0.0625], device=dev)
    w = torch.tensor([1.3, 0.4, 20.0, 2.2], device=dev)
    grads = {}
    for how in ("fused", "torch"):
        m.zero_grad(set_to_none=True)
        out, info = m(x, None, None, None)
        if how == "fused":
            loss = ops.ign_loss(info.shapelet_preds, info.dnn_preds, ya, beta, reg=info.loss, class_weight=w, label_smoothing=eps,
                                y_b=yb, lam=lam)[0]
        else:
            loss = (mix_cross_entropy(out, ya, yb, lam, w, eps) + info.loss.mean()
                    + beta * mix_cross_entropy(info.shapelet_preds, ya, yb, lam, w, eps))
        loss.backward()
        grads[how] = (loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    _SEEN["mix_step.loss"] = parity("mix_step.loss", grads["fused"][0], grads["torch"][0], tol=1e-5, kind="scale",
                                    ref_is="torch composition on the GPU")
    assert grads["fused"][1].keys() == grads["torch"][1].keys()
    for n, ref in grads["torch"][1].items():
        _SEEN[f"mix_step.grad.{n}"] = parity(f"mix_step.grad.{n}", grads["fused"][1][n], ref, tol=1e-5, kind="scale",
                                             ref_is="torch composition on the GPU")
