"""The weighted / label-smoothed loss tail (ign_loss_w_fwd_bwd_reg behind ops.ign_loss(class_weight=, label_smoothing=)) on the
GPU: against float64 (gini gate + F.cross_entropy(weight=, label_smoothing=) + autograd on the CPU), bitwise repeatability, the gate
left as it is, the default call left as it is, the scale invariance of the weights, one model step against the torch composition,
and the harness with the two flags, eager and captured.  Logits are randn * 3, the weights lie in [0.2, 5] with one class at 50
times the largest of the others, the last class never occurs in the batch, beta = 0.37 and a regulariser value is given."""
import pytest
import torch
import torch.nn.functional as F
from conftest import make_cfg, parity

pytestmark = pytest.mark.gpu
BETA, REG = 0.37, 0.125
# (1,2) smallest; (5,3) a small narrow row; (257,16) thread 0 takes a second row and the register row is full; (17,17) the
# narrowest wave-per-row case, one wave takes a second row; (17,65) one lane in a second chunk; (17,256) every chunk full
SHAPES = [(1, 2), (5, 3), (257, 16), (17, 17), (17, 65), (17, 256)]
OPTIONS = [(True, 0.0), (True, 0.1), (False, 0.1)]               # (weights given, label smoothing)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import speech_imagery_eeg_amd  # noqa: F401
    return torch.device("cuda:0")


def _case(B, N):
    """-> host tensors (s, d, y, w): class 0 is the heavy one and occurs, class N - 1 does not occur.
    A batch of ONE row: gdnn = (1 - eta) * go, and that row alone sets the scale gdnn is judged against.  The fp32 gate rule (kept
    bitwise ign_gate_fwd's) carries about N ulp(1) = 2.4e-7 of absolute error in eta, so 1e-5 of scale can be asked of it only while
    1 - eta >= 0.024; the single row is drawn again (same generator) until its float64 1 - eta is at least 0.1.  The first
    randn * 3 draw at (1, 2) has 1 - eta = 0.0034: the fp32 gate arithmetic alone, evaluated on the CPU, is then 6.4e-5 off in
    1 - eta, which is what gdnn showed on the GPU.  Larger batches have rows of every eta and need no such rule."""
    g = torch.Generator().manual_seed(1000 * N + B)
    while True:
        s, d = torch.randn(B, N, generator=g) * 3, torch.randn(B, N, generator=g) * 3
        q = torch.softmax(s.double(), -1)
        if B > 1 or float(1 - ((q * q).sum() * N - 1) / (N - 1)) >= 0.1:
            break
    y = torch.randint(0, N - 1, (B,), generator=g)
    y[0] = 0
    w = 0.2 + 4.8 * torch.rand(N, generator=g)
    w[0] = 50.0 * w[1:].max()
    return s, d, y, w


def _oracle(s, d, y, w, eps, upstream=1.0):
    s = s.double().requires_grad_(True)
    d = d.double().requires_grad_(True)
    N = s.shape[1]
    q = torch.softmax(s, -1)
    eta = ((q * q).sum(-1, keepdim=True) * N - 1) / (N - 1)
    out = eta * s + (1 - eta) * d
    w = None if w is None else w.double()
    loss = F.cross_entropy(out, y, weight=w, label_smoothing=eps) + BETA * F.cross_entropy(s, y, weight=w, label_smoothing=eps) + REG
    (loss * upstream).backward()
    return loss.detach(), out.detach(), eta.detach(), s.grad, d.grad


def _run(dev, s, d, y, w, eps, upstream=None, spell_out=False):
    from ign_hip import ops
    sv, dv = s.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    reg = torch.tensor([REG], device=dev)
    kw = {}
    if w is not None or eps or spell_out:
        kw.update(class_weight=None if w is None else w.to(dev), label_smoothing=eps)
    loss, out, eta = ops.ign_loss(sv, dv, y.to(dev), BETA, reg=reg, **kw)
    (loss if upstream is None else loss * upstream).backward()
    return loss.detach(), out, eta, sv.grad, dv.grad


@pytest.fixture(scope="module")
def oracle():
    """float64 references, computed once per (shape, options)"""
    memo = {}

    def get(B, N, weights, eps):
        key = (B, N, weights, eps)
        if key not in memo:
            s, d, y, w = _case(B, N)
            memo[key] = _oracle(s, d, y, w if weights else None, eps)
        return memo[key]
    return get


# ---------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("weights,eps", OPTIONS)
@pytest.mark.parametrize("B,N", SHAPES)
def test_weighted_tail_vs_float64(oracle, B, N, weights, eps):
    dev = _dev()
    s, d, y, w = _case(B, N)
    l64, o64, e64, gs64, gd64 = oracle(B, N, weights, eps)
    loss, out, eta, gs, gd = _run(dev, s, d, y, w if weights else None, eps)
    tag = f"cew_b{B}_n{N}_w{int(weights)}_e{eps}"
    parity(tag + ".loss", loss, l64, tol=1e-5, kind="elem", ref_is="float64")
    parity(tag + ".out", out, o64, tol=1e-5, kind="elem", ref_is="float64")
    parity(tag + ".eta", eta, e64, tol=1e-5, kind="elem", ref_is="float64")
    parity(tag + ".gsbm", gs, gs64, tol=1e-5, kind="scale", ref_is="float64")
    parity(tag + ".gdnn", gd, gd64, tol=1e-5, kind="scale", ref_is="float64")


@pytest.mark.parametrize("B,N", [(5, 3), (17, 65)])
def test_weighted_tail_with_an_upstream_gradient(B, N):
    dev = _dev()
    s, d, y, w = _case(B, N)
    _, _, _, gs64, gd64 = _oracle(s, d, y, w, 0.1, upstream=-2.5)
    _, _, _, gs, gd = _run(dev, s, d, y, w, 0.1, upstream=-2.5)
    parity(f"cew_up_n{N}.gsbm", gs, gs64, tol=1e-5, kind="scale", ref_is="float64")
    parity(f"cew_up_n{N}.gdnn", gd, gd64, tol=1e-5, kind="scale", ref_is="float64")


# ---------------------------------------------------------------- 2. bitwise repeatability
@pytest.mark.parametrize("B,N", [(257, 16), (17, 65)])
def test_two_calls_are_bitwise_equal(B, N):
    dev = _dev()
    s, d, y, w = _case(B, N)
    a, b = _run(dev, s, d, y, w, 0.1), _run(dev, s, d, y, w, 0.1)
    for name, u, v in zip(("loss", "out", "eta", "gsbm", "gdnn"), a, b):
        assert torch.equal(u, v), name


# ---------------------------------------------------------------- 3. the gate is ign_gate_fwd's
@pytest.mark.parametrize("B,N", [(1, 2), (5, 3), (257, 16)])
def test_gate_is_unchanged_up_to_16_classes(B, N):
    dev = _dev()
    from ign_hip import ops
    s, d, y, w = _case(B, N)
    _, out, eta, _, _ = _run(dev, s, d, y, w, 0.1)
    out_g, eta_g = ops.gini_gate(s.to(dev), d.to(dev))
    assert torch.equal(out, out_g) and torch.equal(eta, eta_g)


# ---------------------------------------------------------------- 4. the default is today's call
@pytest.mark.parametrize("B,N", [(257, 16), (17, 65)])
def test_default_is_untouched(B, N):
    dev = _dev()
    s, d, y, _ = _case(B, N)
    a, b = _run(dev, s, d, y, None, 0.0), _run(dev, s, d, y, None, 0.0, spell_out=True)
    for name, u, v in zip(("loss", "out", "eta", "gsbm", "gdnn"), a, b):
        assert torch.equal(u, v), name
    l64, _, _, gs64, gd64 = _oracle(s, d, y, None, 0.0)          # and it is still the plain cross-entropy
    parity(f"cew_default_n{N}.loss", a[0], l64, tol=1e-5, kind="elem", ref_is="float64")
    parity(f"cew_default_n{N}.gsbm", a[3], gs64, tol=1e-5, kind="scale", ref_is="float64")


# ---------------------------------------------------------------- 5. a common scale of the weights cancels
@pytest.mark.parametrize("B,N", [(257, 16), (17, 65)])
def test_scale_invariance(B, N):
    dev = _dev()
    s, d, y, w = _case(B, N)
    a, b = _run(dev, s, d, y, w, 0.1), _run(dev, s, d, y, 4 * w, 0.1)
    parity(f"cew_scale_n{N}.loss", b[0], a[0], tol=1e-5, kind="elem", ref_is="the same call with w / 4")
    parity(f"cew_scale_n{N}.gsbm", b[3], a[3], tol=1e-5, kind="scale", ref_is="the same call with w / 4")
    parity(f"cew_scale_n{N}.gdnn", b[4], a[4], tol=1e-5, kind="scale", ref_is="the same call with w / 4")


# ---------------------------------------------------------------- 6. one model step
def test_model_step_equals_the_torch_composition():
    """A tiny InterpGN (FCN expert): one backward pass under the fused weighted tail, one under the loss composed from
    F.cross_entropy(weight=, label_smoothing=) on the model's own GPU logits.  Only the tail differs, so the parameter gradients
    agree to 1e-5 of each gradient's scale."""
    dev = _dev()
    from ign_hip import ops
    from models.InterpGN import InterpGN
    B, T, C, N, eps = 6, 40, 3, 4, 0.1
    torch.manual_seed(0)
    m = InterpGN(make_cfg(enc_in=C, seq_len=T, num_class=N, c_out=N, dec_in=C)).to(dev).train()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, T, C, generator=g).to(dev)
    y = torch.tensor([0, 1, 2, 0, 1, 0], device=dev)              # class 3 does not occur
    w = torch.tensor([1.3, 0.4, 20.0, 2.2], device=dev)
    grads = {}
    for how in ("fused", "torch"):
        m.zero_grad(set_to_none=True)
        out, info = m(x, None, None, None)
        if how == "fused":
            loss = ops.ign_loss(info.shapelet_preds, info.dnn_preds, y, BETA, reg=info.loss, class_weight=w, label_smoothing=eps)[0]
        else:
            loss = (F.cross_entropy(out, y, weight=w, label_smoothing=eps) + info.loss.mean()
                    + BETA * F.cross_entropy(info.shapelet_preds, y, weight=w, label_smoothing=eps))
        loss.backward()
        grads[how] = (loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    parity("cew_step.loss", grads["fused"][0], grads["torch"][0], tol=1e-5, kind="elem", ref_is="torch composition on the GPU")
    assert grads["fused"][1].keys() == grads["torch"][1].keys()
    for n, ref in grads["torch"][1].items():
        parity(f"cew_step.grad.{n}", grads["fused"][1][n], ref, tol=1e-5, kind="scale", ref_is="torch composition on the GPU")


# ---------------------------------------------------------------- 7. the harness, eager and captured
def test_harness_with_both_flags_eager_and_hipgraph(tmp_path, monkeypatch):
    """`run.py --class_weight balanced --label_smoothing 0.1` on the SYNTH provider, eager and with --hipgraph: the criterion of
    test_gpu_driver.py::test_hipgraph_harness_run_equals_the_eager_run (validation numbers and final weights within 1e-5), and the
    per-class metrics of Experiment.test."""
    _dev()
    import run
    from exp.experiment_classification import Experiment
    monkeypatch.chdir(tmp_path)
    outs = {}
    for mode in ("eager", "graph"):
        argv = ["--model", "InterpGN", "--dnn_type", "FCN", "--data", "SYNTH", "--synthetic", "104,6,100,4", "--dataset", "cw" + mode,
                "--batch_size", "32", "--amp", "--train_epochs", "2", "--num_workers", "0", "--seed", "0", "--beta_schedule", "cosine",
                "--lr_decay", "--patience", "10", "--class_weight", "balanced", "--label_smoothing", "0.1"] \
            + (["--hipgraph"] if mode == "graph" else [])
        a = run.get_args(argv)
        run.set_seed(0)
        e = Experiment(a)
        assert e.class_weight is not None and e.class_weight.shape == (4,) and e.class_weight.is_cuda and e.label_smoothing == 0.1
        weight_address = e.class_weight.data_ptr()
        vals, orig = [], e.validation

        def rec(orig=orig, vals=vals):
            r = orig()
            vals.append(r)
            return r
        e.validation = rec
        torch.manual_seed(123)
        e.train()
        assert e.class_weight.data_ptr() == weight_address           # allocated once: the captured step replays this tensor
        outs[mode] = (vals, {k: v.detach().float().cpu().clone() for k, v in e.model.state_dict().items()})
        if mode == "graph":
            assert getattr(e, "_graphed", None) is not None and e.optimizer.capturable      # the graph path really ran
        _, res, _ = e.test(save_csv=False)
        n = len(e.test_data)
        assert res.confusion.shape == (4, 4) and res.confusion.dtype == torch.int64 and int(res.confusion.sum()) == n
        rows = res.confusion.sum(1).double()
        seen = rows > 0
        assert torch.allclose(res.recall, torch.where(seen, res.confusion.diag().double() / rows.clamp(min=1), rows * 0))
        assert res.balanced_accuracy == pytest.approx(float(res.recall[seen].mean())) and 0.0 <= res.macro_f1 <= 1.0
        assert res.accuracy == pytest.approx(float(res.confusion.diag().sum()) / n)
    for (la, aa), (lb, ab) in zip(*[o[0] for o in outs.values()]):
        assert abs(la - lb) <= 1e-5 * max(1.0, abs(la)) and aa == ab
    for k, v in outs["eager"][1].items():
        w = outs["graph"][1][k]
        assert float((v - w).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max())), k
