"""SBM bilinear head on the fp32 matrix-core kernels (ops.sbm_bilinear, include/ign_abi.h ign_sbm_bilinear_*): output and all three
gradients against a float64 restatement of nn.Bilinear (no bias) at small and full size; memory without any (B,F,F) temporary;
bitwise-reproducible backward; only the gradients asked for; the model routes through the kernels (eager, autocast, dropout,
hipGraph).  Tolerance 1e-4 (north_star) through conftest.parity."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import golden, make_cfg, parity, sd_from

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def _inputs(B, F_, N, dev, seed):
    """u != v, W with nn.Bilinear's init scale, a random upstream gradient"""
    g = torch.Generator().manual_seed(seed)
    u, v = torch.randn(B, F_, generator=g), torch.randn(B, F_, generator=g)
    w = (torch.rand(N, F_, F_, generator=g) * 2 - 1) / F_ ** 0.5
    gout = torch.randn(B, N, generator=g)
    return [t.to(dev) for t in (u, v, w, gout)]


def _closed_forms64(u, v, w, gout):
    """float64 out, gu, gv, gw from the closed forms, by matmuls (no (B,F,F) tensor)"""
    u, v, w, g = (t.double() for t in (u, v, w, gout))
    T = torch.stack([u @ w[n] for n in range(w.shape[0])], 1)              # (B,N,F)
    out = (T * v[:, None, :]).sum(-1)
    gu = sum((g[:, n, None] * v) @ w[n].T for n in range(w.shape[0]))
    gv = (g[:, :, None] * T).sum(1)
    gw = torch.stack([(g[:, n, None] * u).T @ v for n in range(w.shape[0])])
    return out, gu, gv, gw


def _run(u, v, w, gout, need=(True, True, True)):
    from ign_hip import ops
    ts = [t.detach().clone().requires_grad_(r) for t, r in zip((u, v, w), need)]
    out = ops.sbm_bilinear(*ts)
    out.backward(gout)
    return out.detach(), [t.grad for t in ts]


def _check(label, B, F_, N, seed):
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    u, v, w, gout = _inputs(B, F_, N, dev, seed)
    out, (gu, gv, gw) = _run(u, v, w, gout)
    ref = _closed_forms64(u, v, w, gout)
    for name, got, r in zip(("out", "grad u", "grad v", "grad w"), (out, gu, gv, gw), ref):
        parity(f"{label}: {name}", got, r, kind="scale", ref_is="float64 restatement")


def test_closed_forms_equal_float64_bilinear_autograd():
    """The restatement the other tests use is nn.Bilinear's own forward and autograd (float64, u != v, bias off)."""
    torch.manual_seed(0)
    u, v = torch.randn(5, 11, dtype=torch.float64), torch.randn(5, 11, dtype=torch.float64)
    w = torch.randn(3, 11, 11, dtype=torch.float64)
    g = torch.randn(5, 3, dtype=torch.float64)
    ts = [t.clone().requires_grad_() for t in (u, v, w)]
    out = F.bilinear(*ts)
    out.backward(g)
    for got, r in zip(_closed_forms64(u, v, w, g), (out.detach(), *[t.grad for t in ts])):
        torch.testing.assert_close(got, r, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("B,F_,N", [(1, 1, 1), (3, 72, 4), (8, 130, 3), (32, 360, 4), (64, 1000, 7)])
def test_op_matches_float64(B, F_, N):
    _check(f"B{B} F{F_} N{N}", B, F_, N, seed=B * 131 + F_ + N)


@pytest.mark.parametrize("F_", [2440, 7320])
def test_full_size_matches_float64(F_):
    """B 256 at F 2440 (InterpGN on CHISCO) and F 7320 (SBM / LTS 6x10 on CHISCO), N 3"""
    _check(f"B256 F{F_} N3", 256, F_, 3, seed=F_)


def test_memory_has_no_f_squared_temporary_beyond_the_weight_gradient():
    """fwd + bwd at (256, 7320, 3): nn.Bilinear's backward writes a 54.9 GB (B,F,F) temporary per class; here the extra memory
    is the weight gradient, T (B,N,F) and small buffers."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    B, F_, N = 256, 7320, 3
    u, v, w, gout = _inputs(B, F_, N, dev, seed=5)
    u.requires_grad_(); v.requires_grad_(); w.requires_grad_()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = ops.sbm_bilinear(u, v, w)
    out.backward(gout)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    bound = w.numel() * 4 + B * N * F_ * 4 + (64 << 20)
    assert extra <= bound, f"{extra / 2**20:.1f} MiB > {bound / 2**20:.1f} MiB"
    assert torch.isfinite(u.grad).all() and torch.isfinite(v.grad).all() and torch.isfinite(w.grad).all()


def test_backward_is_bitwise_reproducible():
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    u, v, w, gout = _inputs(96, 1000, 3, dev, seed=8)
    runs = [_run(u, v, w, gout) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)


def test_no_grad_forward_equals_the_autograd_forward():
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    u, v, w, _ = _inputs(5, 77, 3, dev, seed=2)
    w.requires_grad_()
    with torch.no_grad():
        a = ops.sbm_bilinear(u, v, w)
    b = ops.sbm_bilinear(u, v, w)
    assert b.requires_grad and not a.requires_grad
    assert torch.equal(a, b.detach())


@pytest.mark.parametrize("need", [(True, True, False), (True, False, False), (False, True, True)])
def test_partial_gradients_are_unchanged(need):
    """W frozen (no dW GEMM), only u requiring grad (no T saved), or u frozen: what is computed equals the full backward."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    u, v, w, gout = _inputs(40, 300, 3, dev, seed=4)
    out_all, grads_all = _run(u, v, w, gout)
    out, grads = _run(u, v, w, gout, need)
    assert torch.equal(out, out_all)
    for g, ga, n in zip(grads, grads_all, need):
        assert (g is not None) == n
        if n:
            assert torch.equal(g, ga)


def _sbm(dev, **kw):
    from models.Shapelet import ShapeBottleneckModel
    g = golden("sbm_bilinear")
    k = int(g["num_shapelet"])
    m = ShapeBottleneckModel(make_cfg(sbm_cls="bilinear", **kw), [k] * 6, [0.05, 0.1, 0.2, 0.3, 0.5, 0.8])
    m.load_state_dict(sd_from(g))
    return m.to(dev).train(), g


def _no_torch_bilinear(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("torch bilinear called: the head did not take the HIP kernels")
    monkeypatch.setattr(F, "bilinear", boom)
    monkeypatch.setattr(nn.Bilinear, "forward", boom)


def test_model_routes_through_the_kernels_and_matches_the_fixture(monkeypatch):
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    _no_torch_bilinear(monkeypatch)
    m, g = _sbm(dev)
    x, y = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["y"]).to(dev)
    out, info = m(x)
    loss = F.cross_entropy(out, y) + info.loss.mean()
    loss.backward()
    parity("out", out, g["out"], kind="elem", f64=g.get("out64"))
    parity("p", info.p, g["p"], kind="elem")
    parity("d", info.d, g["d"], kind="elem")
    parity("model_loss", info.loss, g["model_loss"], kind="elem")
    parity("train_loss", loss, g["train_loss"], kind="elem")
    gmax = max(float(np.abs(g[k]).max()) for k in g if k.startswith("grad."))
    for n, p in m.named_parameters():
        parity("grad." + n, p.grad, g["grad." + n], kind="scale", floor=1e-4 * gmax, f64=g.get("grad64." + n))
    m.eval()
    with torch.no_grad():
        oe, _ = m(x)
    parity("eval out", oe, g["out"], kind="elem", f64=g.get("out64"))


def test_model_inside_autocast_keeps_the_output_dtype(monkeypatch):
    """Inside torch.autocast(cuda, bf16) the head's output has the dtype the nn.Bilinear path gives (nn.Bilinear promotes to its
    widest input: fp32) and equals that path's value."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    m, g = _sbm(dev)
    x = torch.from_numpy(g["x"]).to(dev)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        _, info = m(x)
        p = info.p.detach()
        ref = m.output_layer(p) + m.output_bilinear(p, p)            # the torch path of head() with dropout 0
        _no_torch_bilinear(monkeypatch)
        got = m.head(p)
        out, _ = m(x)
    assert got.dtype == ref.dtype and out.dtype == ref.dtype, (got.dtype, out.dtype, ref.dtype)
    parity("autocast head", got, ref, kind="scale", ref_is="nn.Bilinear path under autocast")
    parity("autocast out vs fp32 fixture", out, g["out"], tol=5e-2, kind="elem", ref_is="fp32 fixture (bf16 linear term)")


def test_dropout_masks_and_result_equal_the_nn_bilinear_path():
    """dropout 0.3 in training: the head draws its three masks in the reference's order, so with one seed the kernel path and the
    nn.Bilinear path give the same output and the same gradients."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    m, _ = _sbm(dev, dropout=0.3)
    p0 = torch.rand(16, m.total_shapelets, generator=torch.Generator().manual_seed(3)).to(dev)
    r = torch.randn(16, 4, generator=torch.Generator().manual_seed(4)).to(dev)
    res = {}
    for path in ("kernel", "torch"):
        mm = copy.deepcopy(m)
        p = p0.clone().requires_grad_()
        torch.manual_seed(11)
        if path == "kernel":
            out = mm.head(p)
        else:
            out = mm.output_layer(mm.dropout(p)) + mm.output_bilinear(mm.dropout(p), mm.dropout(p))
        (out * r).sum().backward()
        res[path] = (out.detach(), p.grad, mm.output_layer.weight.grad, mm.output_bilinear.weight.grad)
    for name, a, b in zip(("out", "grad p", "grad output_layer", "grad output_bilinear"), res["kernel"], res["torch"]):
        parity(f"dropout 0.3: {name}", a, b, kind="scale", ref_is="nn.Bilinear path, same seed")


def test_graphed_sbm_bilinear_step_equals_eager():
    """One SBM step with the bilinear head (fused SBM node, head kernels, backward, capturable flat Adam) captured as a hipGraph
    and replayed on 3 batches walks the eager parameter trajectory (mirrors test_graphed_sbm_attention_step_equals_eager)."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip.ddp import FlatAdam, FlatParamBucket
    from ign_hip.graph import GraphedTrainStep
    from models.Shapelet import ShapeBottleneckModel
    torch.manual_seed(0)
    base = ShapeBottleneckModel(make_cfg(sbm_cls="bilinear"))
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(8, 100, 6, generator=g).to(dev) for _ in range(4)]
    ys = [(torch.arange(8) % 4).to(dev) for _ in range(4)]
    finals = {}
    for mode in ("eager", "graph"):
        model = copy.deepcopy(base).to(dev).train()
        bucket = FlatParamBucket(model, 1)
        opt = FlatAdam(bucket, lr=5e-3, capturable=(mode == "graph"))

        def step(x, y, model=model, bucket=bucket, opt=opt):
            out, info = model(x)
            loss = F.cross_entropy(out, y) + info.loss.mean()
            loss.backward()
            opt.step()
            bucket.zero_grad()
            return loss.detach()

        if mode == "graph":
            sd = copy.deepcopy(model.state_dict())
            stepper = GraphedTrainStep(step, (xs[0], ys[0]), warmup=2)
            model.load_state_dict(sd)
            opt.exp_avg.zero_(); opt.exp_avg_sq.zero_(); opt.step_dev.zero_()
        else:
            stepper = step
        losses = [float(stepper(x, y)) for x, y in zip(xs[1:], ys[1:])]
        torch.cuda.synchronize()
        finals[mode] = (losses, {k: v.detach().clone() for k, v in model.state_dict().items()})
    for a, b in zip(finals["eager"][0], finals["graph"][0]):
        assert a == a and abs(a - b) <= 1e-6 * max(1.0, abs(a)), (finals["eager"][0], finals["graph"][0])
    for k, v in finals["eager"][1].items():
        w = finals["graph"][1][k]
        if v.dtype.is_floating_point:
            assert float((v - w).abs().max()) <= 1e-6 * max(1.0, float(v.abs().max())), k
    assert finals["eager"][1]["output_bilinear.weight"].ne(base.state_dict()["output_bilinear.weight"].to(dev)).any()
