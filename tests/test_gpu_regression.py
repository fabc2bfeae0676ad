"""The regression task on the HIP path: the CRPS loss tail kernels (ign_crps_fwd_bwd, ign_loss_crps_fwd_bwd_reg) against a
float64 torch restatement and the reference's fixtures, their launch count, capture / replay, the reference's InterpGN
regression train step replayed on the flat Adam, and RegressionExperiment end to end."""
import glob
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT, golden, make_cfg, parity, sd_from

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "speech-imagery-eeg_amd")
BS = [1, 7, 32, 256, 1000]
NS = [2, 3, 10, 16, 17, 64, 256]
SHAPELET_LENGTHS = [0.05, 0.1, 0.2, 0.3, 0.5, 0.8]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import speech_imagery_eeg_amd  # noqa: F401
    return torch.device("cuda:0")


def _edges(N, lo=-2.0, hi=2.0):
    """Monash-style upper edges: N values, the last +inf; float32-exact so that a target can sit on an edge"""
    e = torch.linspace(lo, hi, N + 1).float().double()
    e[-1] = float("inf")
    return e[1:]


def _targets(B, edges, g):
    y = torch.randn(B, generator=g) * 1.5
    fin = edges[:-1]
    if B > 1 and len(fin):
        y[0] = float(fin[len(fin) // 2])              # on an edge: counts as >=
    if B > 2:
        y[1] = -10.0                                  # below the first edge
    if B > 3:
        y[2] = 10.0                                   # above the last finite edge
    return y.float()


def _crps64(z, y, edges):
    F = torch.cumsum(torch.softmax(z, dim=1), dim=1)
    H = (edges.unsqueeze(0) >= y.double().reshape(-1, 1)).double()
    return ((F - H) ** 2).sum(1).mean()


def _gate64(s, d):
    N = s.shape[1]
    q = torch.softmax(s, -1)
    eta = ((q * q).sum(-1, keepdim=True) * N - 1) / (N - 1)
    return eta * s + (1 - eta) * d, eta


# ------------------------------------------------------------------------------------------------------------ kernels vs float64
@pytest.mark.parametrize("N", NS)
def test_crps_loss_vs_float64(N):
    dev = _dev()
    from ign_hip import ops
    edges = _edges(N)
    for B in BS:
        g = torch.Generator().manual_seed(1000 * N + B)
        z = torch.randn(B, N, generator=g) * 2.5
        y = _targets(B, edges, g)
        z64 = z.double().requires_grad_(True)
        l64 = _crps64(z64, y, edges)
        l64.backward()
        res = []
        for _ in range(2):
            zv = z.to(dev).requires_grad_(True)
            loss = ops.crps_loss(zv, y.to(dev), edges.to(dev))
            ops.backward(loss)
            res.append((loss.detach().clone(), zv.grad.clone()))
        parity(f"crps_n{N}_b{B}.loss", res[0][0], l64.detach(), kind="elem", ref_is="float64")
        parity(f"crps_n{N}_b{B}.grad", res[0][1], z64.grad, kind="scale", floor=1e-7, ref_is="float64")
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), "two calls differ"
        # loss.backward() (a root gradient that is not the cached unit) gives the same gradient
        zv = z.to(dev).requires_grad_(True)
        ops.crps_loss(zv, y.to(dev), edges.to(dev)).backward()
        assert torch.equal(zv.grad, res[0][1])


@pytest.mark.parametrize("N", NS)
def test_ign_crps_loss_vs_float64(N):
    dev = _dev()
    from ign_hip import ops
    edges = _edges(N)
    for B in BS:
        g = torch.Generator().manual_seed(7000 * N + B)
        s = torch.randn(B, N, generator=g) * 2.5
        d = torch.randn(B, N, generator=g) * 2.5
        y = _targets(B, edges, g)
        for beta in (0.0, 0.5, 1.0):
            for reg in (None, 0.375):
                s64, d64 = s.double().requires_grad_(True), d.double().requires_grad_(True)
                o64, e64 = _gate64(s64, d64)
                l64 = _crps64(o64, y, edges) + beta * _crps64(s64, y, edges) + (reg or 0.0)
                l64.backward()
                sv, dv = s.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
                r = None if reg is None else torch.tensor([reg], device=dev)
                loss, out, eta = ops.ign_crps_loss(sv, dv, y.to(dev), edges.to(dev), beta, reg=r)
                ops.backward(loss)
                tag = f"ign_crps_n{N}_b{B}_beta{beta}_reg{reg}"
                parity(tag + ".loss", loss, l64.detach(), kind="elem", ref_is="float64")
                parity(tag + ".out", out, o64.detach(), kind="elem", ref_is="float64")
                parity(tag + ".eta", eta, e64.detach(), kind="elem", ref_is="float64")
                parity(tag + ".gsbm", sv.grad, s64.grad, kind="scale", floor=1e-7, ref_is="float64")
                parity(tag + ".gdnn", dv.grad, d64.grad, kind="scale", floor=1e-7, ref_is="float64")
                # the mixture and gate are ign_gate_fwd's, bit for bit
                og, eg = ops.gini_gate(s.to(dev), d.to(dev))
                assert torch.equal(out, og) and torch.equal(eta, eg), tag
                # loss.backward() == ops.backward(loss), and a second call is bitwise the same
                sv2, dv2 = s.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
                loss2 = ops.ign_crps_loss(sv2, dv2, y.to(dev), edges.to(dev), beta, reg=r)[0]
                loss2.backward()
                assert torch.equal(loss2, loss) and torch.equal(sv2.grad, sv.grad) and torch.equal(dv2.grad, dv.grad), tag


@pytest.mark.parametrize("N", [2, 10, 39])
def test_crps_loss_matches_reference_fixture(N):
    dev = _dev()
    from ign_hip import ops
    g = golden("crps_loss")
    z = torch.from_numpy(g[f"n{N}_logits"]).to(dev).requires_grad_(True)
    loss = ops.crps_loss(z, torch.from_numpy(g[f"n{N}_target"]).to(dev), torch.from_numpy(g[f"n{N}_edges"]).to(dev))
    ops.backward(loss)
    parity(f"crps_ref_n{N}.loss", loss, np.float64(g[f"n{N}_loss"]), kind="elem")
    parity(f"crps_ref_n{N}.grad", z.grad, g[f"n{N}_grad"], kind="scale", floor=1e-7)


def test_crps_bad_arguments_raise():
    dev = _dev()
    from ign_hip import _lib, ops
    z = torch.randn(4, 300, device=dev)
    with pytest.raises(_lib.IgnError, match="N=300"):
        ops.crps_loss(z, torch.zeros(4, device=dev), torch.zeros(300, dtype=torch.float64, device=dev))
    with pytest.raises(_lib.IgnError, match="bin edges"):
        ops.crps_loss(z[:, :10], torch.zeros(4, device=dev), torch.zeros(9, dtype=torch.float64, device=dev))
    with pytest.raises(_lib.IgnError):
        ops.crps_loss(z[:, :10].cpu(), torch.zeros(4), torch.zeros(10, dtype=torch.float64))


def test_bf16_logits_are_cast_to_fp32():
    dev = _dev()
    from ign_hip import ops
    edges = _edges(10).to(dev)
    z = torch.randn(32, 10, device=dev)
    y = torch.randn(32, device=dev)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        zb = z.bfloat16()
        loss = ops.crps_loss(zb, y, edges)
    assert loss.dtype == torch.float32
    assert torch.equal(loss, ops.crps_loss(zb.float(), y, edges))


# ------------------------------------------------------------------------------------------------------------ launches, capture
def _device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [ev.name for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA")
             and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower()]
    if not names:
        pytest.skip("torch.profiler reported no device events here")
    return names


@pytest.mark.parametrize("N", [10, 64])
def test_one_launch_per_loss_call(N):
    dev = _dev()
    from ign_hip import ops
    edges = _edges(N).to(dev)
    z = torch.randn(32, N, device=dev, requires_grad=True)
    s = torch.randn(32, N, device=dev, requires_grad=True)
    d = torch.randn(32, N, device=dev, requires_grad=True)
    y = torch.randn(32, device=dev)
    reg = torch.tensor([0.25], device=dev)
    unit = ops.unit_grad(dev)

    def crps():
        loss = ops.crps_loss(z, y, edges)
        torch.autograd.grad(loss, [z], grad_outputs=unit)          # the gradient is the saved one: no launch

    def ign():
        loss = ops.ign_crps_loss(s, d, y, edges, 0.5, reg=reg)[0]
        torch.autograd.grad(loss, [s, d], grad_outputs=unit)

    k1, k2 = _device_kernels(crps), _device_kernels(ign)
    assert len(k1) == 1 and "crps_kernel" in k1[0], k1
    assert len(k2) == 1 and "ign_crps_kernel" in k2[0], k2


def test_capture_and_replay_equal_eager():
    dev = _dev()
    from ign_hip import ops
    N, B = 10, 48
    edges = _edges(N).to(dev)
    reg = torch.tensor([0.5], device=dev)

    def inputs(seed):
        g = torch.Generator().manual_seed(seed)
        return [(torch.randn(B, N, generator=g) * 2).to(dev), (torch.randn(B, N, generator=g) * 2).to(dev),
                torch.randn(B, generator=g).to(dev)]

    def run(s, d, y):
        l1 = ops.crps_loss(s, y, edges)
        l2, out, eta = ops.ign_crps_loss(s, d, y, edges, 0.75, reg=reg)
        return l1, l2, out, eta

    static = inputs(5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(*static)
    for seed in (11, 12):
        new = inputs(seed)
        for st, v in zip(static, new):
            st.copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, run(*new)):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ reference train step
def _sd32(g, prefix):
    return {k: (v.float() if v.is_floating_point() else v) for k, v in sd_from(g, prefix).items()}


def _compact_close(label, t, g, prefix, name, tol=1e-4):
    """make_golden.grads_compact's layout: prefix + '.' + name in full, or prefix + 'norm.' / 'sample.' + name"""
    if f"{prefix}.{name}" in g:
        parity(f"{label}.{name}", t, g[f"{prefix}.{name}"], kind="scale", floor=1e-7, tol=tol)
        return
    flat = t.detach().flatten()
    idx = torch.linspace(0, flat.numel() - 1, min(2048, flat.numel())).long().to(flat.device)
    parity(f"{label}.sample.{name}", flat[idx], g[f"{prefix}sample.{name}"], kind="scale", floor=1e-7, tol=tol)
    nrm = float(flat.double().norm())
    assert abs(nrm - float(g[f"{prefix}norm.{name}"])) <= tol * max(1e-7, nrm), name


def test_train_step_ign_regression_fixture():
    dev = _dev()
    from ign_hip import ops
    from ign_hip.ddp import FlatAdam, FlatParamBucket
    from models.InterpGN import InterpGN
    g = golden("train_step_ign_regression")
    m = InterpGN(make_cfg(num_class=10, c_out=10), num_shapelet=[2] * 6, shapelet_len=SHAPELET_LENGTHS)
    m.load_state_dict(_sd32(g, "sd0."))
    m.to(dev).train()
    bucket = FlatParamBucket(m, 1)
    opt = FlatAdam(bucket, lr=5e-3)
    xs, ys = torch.from_numpy(g["xs"]).to(dev), torch.from_numpy(g["ys"]).to(dev)
    edges = torch.from_numpy(g["edges"]).to(dev)
    beta = float(g["beta"])
    for i in range(3):
        out, info = m(xs[i], torch.ones(xs.shape[1], xs.shape[2], device=dev), None, None)
        loss, mix, eta = ops.ign_crps_loss(info.shapelet_preds, info.dnn_preds, ys[i], edges, beta, reg=info.loss)
        ops.backward(loss)
        if i == 0:
            for k, v in (("out0", mix), ("sbm0", info.shapelet_preds), ("dnn0", info.dnn_preds), ("eta0", eta)):
                parity("reg_step." + k, v, g[k], kind="elem")
            assert torch.equal(mix, out) and torch.equal(eta, info.eta)       # the model's gate and the loss tail's agree
            for n, p in m.named_parameters():
                if n.startswith("deep_model.block") and n.endswith(".0.bias"):
                    continue
                _compact_close("reg_step.grad0", p.grad, g, "grad0.", n)
        parity(f"reg_step.loss{i}", loss, np.float64(g["losses"][i]), kind="elem")
        bucket.allreduce()
        opt.step()
        bucket.zero_grad()
    for k, v in m.state_dict().items():
        if not v.is_floating_point() or (k.startswith("deep_model.block") and (k.endswith(".0.bias") or k.endswith("running_mean"))):
            continue
        if "sd3." + k in g:
            a, b = v.detach().cpu().double().numpy(), g["sd3." + k].astype(np.float64)
        else:
            flat = v.detach().flatten().cpu()
            a = flat[torch.linspace(0, flat.numel() - 1, min(2048, flat.numel())).long()].double().numpy()
            b = g["sd3.sample." + k].astype(np.float64)
        diff = np.abs(a - b)
        bad = diff > (5e-4 + 5e-3 * np.abs(b))
        assert bad.mean() <= 0.05, f"{k}: {bad.mean():.3%} of entries outside tolerance"
        assert diff.max() <= 3 * 2 * 5e-3 + 1e-6, f"{k}: max diff {diff.max():.3e}"


# ------------------------------------------------------------------------------------------------------------ the experiment
def _write_burst(tmp, n_train=96, n_test=32, C=3, T=120):
    """Monash-format set whose target is the amplitude of a planted burst: learnable, so the loss can fall"""
    import speech_imagery_eeg_amd  # noqa: F401
    from data_provider.ts_reader import write_ts
    d = os.path.join(tmp, "Burst")
    os.makedirs(d, exist_ok=True)
    for split, n, seed in (("TRAIN", n_train, 1), ("TEST", n_test, 2)):
        rng = np.random.RandomState(seed)
        amp = rng.rand(n) * 5
        X = []
        for i in range(n):
            x = rng.randn(C, T) * 0.3
            t0 = rng.randint(0, T - 20)
            x[:, t0:t0 + 20] += amp[i]
            X.append(x)
        write_ts(os.path.join(d, f"Burst_{split}.ts"), X, amp, regression=True)
    return d


def _reg_args(tmp, model, epochs=8, extra=()):
    import run
    return run.get_args(["--task_name", "regression", "--data", "Monash", "--model", model, "--dnn_type", "FCN", "--data_root",
                         str(tmp), "--dataset", "Burst", "--train_epochs", str(epochs), "--batch_size", "16", "--seed", "0",
                         "--amp", "--log_interval", "1", "--num_shapelet", "4", "--patience", "100", "--lr", "5e-3"]
                        + list(extra))


@pytest.mark.parametrize("model", ["InterpGN", "SBM", "LTS", "DNN"])
def test_regression_experiment_trains(tmp_path, monkeypatch, model):
    _dev()
    import run
    from exp.experiment_regression import Experiment
    _write_burst(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    run.set_seed(0)
    e = Experiment(_reg_args(tmp_path, model))
    assert e.args.num_class == 10 and e.edges.is_cuda and e.edges.dtype == torch.float64
    epoch_losses = []
    orig = e.train_one_epoch

    def rec(epoch, train_step=0):
        losses, step = orig(epoch, train_step)
        epoch_losses.append(torch.stack(losses).mean().item())
        return losses, step

    monkeypatch.setattr(e, "train_one_epoch", rec)
    e.train()
    assert all(np.isfinite(epoch_losses)) and len(epoch_losses) == 8
    assert min(epoch_losses[-3:]) < epoch_losses[0], epoch_losses
    ck = torch.load(os.path.join(e.checkpoint_dir, "checkpoint.pth"), map_location="cpu", weights_only=True)
    assert list(ck) == list(e.model.state_dict())
    loss, res, df = e.test(result_dir=str(tmp_path / "result"))
    assert isinstance(loss, float) and np.isfinite(loss) and res is None and isinstance(df, dict)
    assert df["pred"].shape == (32, 10) and df["target"].shape == (32,)
    assert glob.glob(str(tmp_path / "result" / f"Burst-0-{model}-*.csv"))


def test_regression_hipgraph_run_equals_eager(tmp_path, monkeypatch):
    _dev()
    import run
    from exp.experiment_regression import Experiment
    _write_burst(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    outs = {}
    for mode in ("eager", "graph"):
        a = _reg_args(tmp_path, "InterpGN", epochs=2, extra=["--hipgraph"] if mode == "graph" else [])
        run.set_seed(0)
        e = Experiment(a)
        e.checkpoint_dir = str(tmp_path / f"ck_{mode}")
        os.makedirs(e.checkpoint_dir, exist_ok=True)
        torch.manual_seed(123)
        e.train()
        outs[mode] = {k: v.detach().float().cpu().clone() for k, v in e.model.state_dict().items()}
        if mode == "graph":
            assert getattr(e, "_graphed", None) is not None
    for k, v in outs["eager"].items():
        assert torch.equal(v, outs["graph"][k]), k


def test_run_py_regression_driver(tmp_path):
    _dev()
    _write_burst(str(tmp_path), n_train=48, n_test=16)
    args = ["--task_name", "regression", "--data", "Monash", "--model", "InterpGN", "--dnn_type", "FCN", "--amp", "--data_root",
            str(tmp_path), "--dataset", "Burst", "--train_epochs", "6", "--patience", "2", "--batch_size", "16", "--seed", "0",
            "--num_shapelet", "3", "--log_interval", "1"]
    r = subprocess.run([sys.executable, os.path.join(PKG, "run.py")] + args, cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"CRPS: ([0-9.eE+-]+)", r.stdout)
    assert m and np.isfinite(float(m.group(1))), r.stdout[-2000:]
    pk = glob.glob(str(tmp_path / "checkpoints" / "InterpGN" / "Burst" / "*" / "test_results.pkl"))
    assert len(pk) == 1 and os.path.exists(os.path.join(os.path.dirname(pk[0]), "checkpoint.pth"))
    with open(pk[0], "rb") as f:
        res = pickle.load(f)
    assert abs(res["test_loss"] - float(m.group(1))) < 1e-5 and res["test_df"]["pred"].shape == (16, 10)
    assert glob.glob(str(tmp_path / "result" / "InterpGN" / "Burst-0-InterpGN-*.csv"))
