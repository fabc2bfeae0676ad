"""Class heads wider than 16 classes (CHISCO's 39 categories, UEA sets with 20-39 classes) on the HIP kernels: the head GEMMs
(ign_head_*) in 16-class chunks, the fused loss tail (ign_loss_*) one wave per row -- against float64, the CPU oracle, the
reference's fixtures, and the launch budget of the 4-class step."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from conftest import ROOT, golden, make_cfg, parity, sd_from

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "speech-imagery-eeg_amd")
BOUND = 256
IGN_E_UNSUP = -1002


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _lib():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    return _lib


def _p(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _within(got, ref64, absref, label, tol=1e-5):
    """|got - ref| <= tol * (|X| |W|^T-style magnitude of the same sum) + 1e-7, element-wise"""
    err = (got.double() - ref64).abs()
    bound = tol * absref + 1e-7
    assert bool((err <= bound).all()), f"{label}: max err {float(err.max()):.3e}, worst ratio {float((err / bound).max()):.2f}"


# ------------------------------------------------------------------------------------------------------------ raw ABI
SHAPES = [(1, 4, 4), (7, 2440, 2440), (256, 2440, 2440), (640, 4, 8), (7, 7320, 7328)]       # (B, F, ldx)


@pytest.mark.parametrize("N", [17, 25, 39, 64, BOUND])
@pytest.mark.parametrize("B,F_,ldx", SHAPES)
def test_head_abi_vs_float64(N, B, F_, ldx):
    dev = _dev()
    L = _lib().lib()
    stream = _lib().stream()
    g = torch.Generator(device="cpu").manual_seed(N * 1000 + B)
    Xp = torch.randn(B, ldx, generator=g).to(dev)
    W = torch.randn(N, F_, generator=g).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    gout = torch.randn(B, N, generator=g).to(dev)
    add = torch.randn(N, F_, generator=g).to(dev)
    scale = torch.tensor([0.37], device=dev)
    X64, W64, g64 = Xp[:, :F_].double(), W.double(), gout.double()

    out = torch.empty(B, N, device=dev)
    assert L.ign_head_fwd(_p(Xp), _p(W), _p(bias), _p(out), B, F_, N, ldx, stream) == 0
    _within(out, X64 @ W64.T + bias.double(), X64.abs() @ W64.abs().T + bias.double().abs(), "out")
    out2 = torch.empty_like(out)
    assert L.ign_head_fwd(_p(Xp), _p(W), _p(bias), _p(out2), B, F_, N, ldx, stream) == 0
    assert torch.equal(out, out2)

    gx_ref, gx_abs = g64 @ W64, g64.abs() @ W64.abs()
    gw_ref, gw_abs = g64.T @ X64, g64.abs().T @ X64.abs()
    gb_ref = g64.sum(0)
    for variant in ("xw", "xw_bias", "xw_add", "x", "w", "w_bias_add"):
        want_x = variant.startswith("x")
        want_w = variant != "x"
        has_b = "bias" in variant
        has_add = "add" in variant
        runs = []
        for _ in range(2):
            gX = torch.full((B, ldx), 7.0, device=dev) if want_x else None
            gW = torch.empty(N, F_, device=dev) if want_w else None
            gb = torch.empty(N, device=dev) if has_b else None
            rc = L.ign_head_bwd_acc(_p(gout), _p(Xp), _p(W), _p(gX), _p(gW), _p(gb), _p(add) if has_add else None,
                                    _p(scale) if has_add else None, B, F_, N, ldx, stream)
            assert rc == 0, (variant, rc)
            runs.append((gX, gW, gb))
        (gX, gW, gb), (gX2, gW2, gb2) = runs
        if want_x:
            _within(gX[:, :F_], gx_ref, gx_abs, f"{variant} gX")
            assert torch.equal(gX, gX2)
            if ldx > F_:
                assert bool((gX[:, F_:] == 7.0).all()), "gX wrote into the row padding"
        if want_w:
            ref = gw_ref + (0.37 * add.double() if has_add else 0.0)
            _within(gW, ref, gw_abs + (0.37 * add.double().abs() if has_add else 0.0), f"{variant} gW")
            assert torch.equal(gW, gW2)
        if has_b:
            _within(gb, gb_ref, g64.abs().sum(0), f"{variant} gbias")
            assert torch.equal(gb, gb2)


def test_head_abi_bound():
    dev = _dev()
    L = _lib().lib()
    B, F_ = 4, 8
    for N, rc_want in ((BOUND, 0), (BOUND + 1, IGN_E_UNSUP)):
        X = torch.randn(B, F_, device=dev)
        W = torch.randn(N, F_, device=dev)
        out = torch.empty(B, N, device=dev)
        g = torch.randn(B, N, device=dev)
        gX, gW = torch.empty(B, F_, device=dev), torch.empty(N, F_, device=dev)
        assert L.ign_head_fwd(_p(X), _p(W), None, _p(out), B, F_, N, F_, None) == rc_want
        assert L.ign_head_bwd(_p(g), _p(X), _p(W), _p(gX), _p(gW), None, B, F_, N, F_, None) == rc_want
        y = torch.zeros(B, dtype=torch.long, device=dev)
        eta, loss2 = torch.empty(B, device=dev), torch.empty(3, device=dev)
        assert L.ign_loss_fwd_bwd(_p(out), _p(out), _p(y), _p(out), _p(eta), _p(loss2), _p(g), _p(g), B, N, 1.0, None) == rc_want
    torch.cuda.synchronize()


def test_head_bwd_batch_bound_above_16_classes():
    """One 16-class chunk of g is staged in LDS above 16 classes: B <= 640 at every N (the N = 16 bound)."""
    dev = _dev()
    L = _lib().lib()
    F_ = 8
    for B, ok in ((640, True), (641, False)):
        X = torch.randn(B, F_, device=dev)
        W = torch.randn(39, F_, device=dev)
        g = torch.randn(B, 39, device=dev)
        gX, gW = torch.empty(B, F_, device=dev), torch.empty(39, F_, device=dev)
        rc = L.ign_head_bwd(_p(g), _p(X), _p(W), _p(gX), _p(gW), None, B, F_, 39, F_, None)
        assert (rc == 0) == ok, (B, rc)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ loss tail
def _loss64(s, d, y, beta, reg):
    s = s.double().cpu().requires_grad_(True)
    d = d.double().cpu().requires_grad_(True)
    N = s.shape[1]
    q = torch.softmax(s, -1)
    eta = ((q * q).sum(-1, keepdim=True) * N - 1) / (N - 1)
    out = eta * s + (1 - eta) * d
    loss = F.cross_entropy(out, y.cpu()) + beta * F.cross_entropy(s, y.cpu()) + reg
    loss.backward()
    return loss.detach(), out.detach(), eta.detach(), s.grad, d.grad


# the wave-per-row kernel's chunk edges at B = 17 (one wave takes a second row): N = 64 is the last full single chunk, 65 puts one
# lane into a second chunk, 256 fills every chunk
_TAIL_CASES = [(B, N) for B in (5, 256, 1500) for N in (17, 39, 100)] + [(17, 64), (17, 65), (17, 256)]


@pytest.mark.parametrize("B,N", _TAIL_CASES)
def test_loss_tail_vs_float64(N, B):
    dev = _dev()
    _lib()
    from ign_hip import ops
    g = torch.Generator().manual_seed(N + B)
    s = (torch.randn(B, N, generator=g) * 3).to(dev)
    d = (torch.randn(B, N, generator=g) * 3).to(dev)
    y = torch.cat([torch.arange(N), torch.randint(0, N, (max(0, B - N),), generator=g)])[:B]
    y = y[torch.randperm(B, generator=g)].to(dev)
    reg = torch.tensor([0.125], device=dev)
    beta = 0.7
    res = []
    for _ in range(2):
        sv, dv = s.clone().requires_grad_(True), d.clone().requires_grad_(True)
        loss, out, eta = ops.ign_loss(sv, dv, y, beta, reg=reg)
        loss.backward()
        res.append((loss.detach(), out, eta, sv.grad, dv.grad))
    l64, o64, e64, gs64, gd64 = _loss64(s, d, y, beta, 0.125)
    loss, out, eta, gs, gd = res[0]
    assert abs(float(loss) - float(l64)) <= 1e-5 * max(1.0, abs(float(l64)))
    parity(f"loss_n{N}.out", out, o64, tol=1e-5, kind="elem", ref_is="float64")
    parity(f"loss_n{N}.eta", eta, e64, tol=1e-5, kind="elem", ref_is="float64")
    parity(f"loss_n{N}.gsbm", gs, gs64, tol=1e-5, kind="scale", ref_is="float64")
    parity(f"loss_n{N}.gdnn", gd, gd64, tol=1e-5, kind="scale", ref_is="float64")
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b), "two calls differ"


# ------------------------------------------------------------------------------------------------------------ models
def _grads_vs(m, ref, label):
    gmax = max(float(q.grad.abs().max()) for q in ref.parameters() if q.grad is not None)
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        if n.startswith("deep_model.block") and n.endswith(".0.bias"):
            assert float(p.grad.abs().max()) <= 1e-6 + 1e-4 * float(q.grad.abs().max()), n
            continue
        if float(q.grad.abs().max()) < 1e-5 * gmax:
            # a true gradient of zero (the key-projection bias of a softmax attention): rounding noise on both sides
            assert float(p.grad.abs().max()) < 1e-5 * gmax, f"{n}: not noise-level"
            continue
        parity(f"{label}.grad.{n}", p.grad, q.grad, kind="scale", floor=1e-7, ref_is="CPU oracle fp32")


@pytest.mark.parametrize("sbm_cls", ["linear", "bilinear", "attention", "lts"])
def test_sbm_39_classes_vs_oracle(sbm_cls):
    dev = _dev()
    _lib()
    from models.Shapelet import ShapeBottleneckModel, DistThresholdSBM
    from oracle import ign_oracle as O
    lts = sbm_cls == "lts"
    cfg = make_cfg(num_class=39, c_out=39, sbm_cls="linear" if lts else sbm_cls)
    ns = [2, 2, 2] if sbm_cls == "bilinear" else [4, 4, 4]
    lens = [0.1, 0.3, 0.6]
    torch.manual_seed(0)
    ref = O.OracleSBM(cfg, ns, lens, lts=lts)
    m = (DistThresholdSBM if lts else ShapeBottleneckModel)(cfg, ns, lens)
    m.load_state_dict(ref.state_dict())
    m.to(dev).train()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(8, 100, 6, generator=g)
    y = torch.randperm(39, generator=g)[:8]
    o_r, i_r = ref(x)
    (F.cross_entropy(o_r, y) + i_r.loss.mean()).backward()
    o, i = m(x.to(dev))
    (F.cross_entropy(o, y.to(dev)) + i.loss.mean()).backward()
    parity(f"sbm39_{sbm_cls}.out", o, o_r.detach(), kind="elem", ref_is="CPU oracle fp32")
    parity(f"sbm39_{sbm_cls}.p", i.p, i_r.p.detach(), kind="elem", ref_is="CPU oracle fp32")
    _grads_vs(m, ref, f"sbm39_{sbm_cls}")


def test_interpgn_fcn_39_classes_vs_oracle_and_gating_value():
    dev = _dev()
    _lib()
    from models.InterpGN import InterpGN
    from ign_hip import ops
    from oracle import ign_oracle as O
    cfg = make_cfg(num_class=39, c_out=39)
    torch.manual_seed(0)
    ref = O.OracleIGN(cfg).train()
    m = InterpGN(cfg)
    m.load_state_dict(ref.state_dict())
    m.to(dev).train()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(16, 100, 6, generator=g)
    y = torch.randperm(39, generator=g)[:16]
    o_r, i_r = ref(x)
    O.train_loss('InterpGN', o_r, i_r, y).backward()
    o, i = m(x.to(dev), None, None, None)
    loss = ops.ign_loss(i.shapelet_preds, i.dnn_preds, y.to(dev), 1.0, reg=i.loss)[0]        # the harness' fp32 route
    loss.backward()
    parity("ign39.out", o, o_r.detach(), kind="elem", ref_is="CPU oracle fp32")
    parity("ign39.eta", i.eta, i_r.eta.detach(), kind="elem", ref_is="CPU oracle fp32")
    _grads_vs(m, ref, "ign39")
    ref.eval()
    m.eval()
    with torch.no_grad():
        og, ig = m(x.to(dev), None, None, None, gating_value=0.05)
        ogr, igr = ref(x, gating_value=0.05)
    parity("ign39.gated_out", og, ogr, kind="elem", ref_is="CPU oracle fp32")
    parity("ign39.gated_eta", ig.eta, igr.eta, kind="elem", ref_is="CPU oracle fp32")


def test_interpgn_39_classes_in_autocast_tracks_the_oracle():
    dev = _dev()
    _lib()
    from models.InterpGN import InterpGN
    from oracle import ign_oracle as O
    cfg = make_cfg(num_class=39, c_out=39)
    torch.manual_seed(0)
    orc = O.OracleIGN(cfg).train()
    m = InterpGN(cfg)
    m.load_state_dict(orc.state_dict())
    m.to(dev).train()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 100, 6, generator=g)
    y = torch.randperm(39, generator=g)[:8]
    with torch.autocast(device_type="cpu", dtype=torch.bfloat16):
        out_o, _ = orc(x)
        loss_o = F.cross_entropy(out_o.float(), y)
    loss_o.backward()
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        out, _ = m(x.to(dev), torch.ones(8, 100, device=dev), None, None)
        loss = F.cross_entropy(out.float(), y.to(dev))
    loss.backward()
    assert float((out.float().cpu() - out_o.float()).abs().max()) < 5e-2 * max(1.0, float(out_o.float().abs().max()))
    assert abs(loss.item() - loss_o.item()) < 3e-2
    go = dict(orc.named_parameters())
    for n, p in m.named_parameters():
        if p.grad is None or n.endswith("0.bias"):
            continue
        ref = go[n].grad.float()
        assert float((p.grad.float().cpu() - ref).norm()) < 0.1 * float(ref.norm()) + 1e-4, n


# ------------------------------------------------------------------------------------------------------------ reference fixtures
def _sd32(g, prefix):
    return {k: (v.float() if v.is_floating_point() else v) for k, v in sd_from(g, prefix).items()}


def _compact_close(label, t, g, prefix, name, tol=1e-4):
    """a tensor stored in full (prefix.name), or as (prefixnorm.name, prefixsample.name: fixed 2048-point sample) --
    make_golden.grads_compact's layout"""
    if f"{prefix}.{name}" in g:
        parity(f"{label}.{name}", t, g[f"{prefix}.{name}"], kind="scale", floor=1e-7, tol=tol)
        return
    flat = t.detach().flatten()
    idx = torch.linspace(0, flat.numel() - 1, min(2048, flat.numel())).long().to(flat.device)
    parity(f"{label}.sample.{name}", flat[idx], g[f"{prefix}sample.{name}"], kind="scale", floor=1e-7, tol=tol)
    nrm = float(flat.double().norm())
    assert abs(nrm - float(g[f"{prefix}norm.{name}"])) <= tol * max(1e-7, nrm), name


def test_ign_fcn_n39_golden():
    dev = _dev()
    _lib()
    from models.InterpGN import InterpGN
    g = golden("ign_fcn_n39")
    m = InterpGN(make_cfg(num_class=39, c_out=39))
    m.load_state_dict(_sd32(g, "sd."))
    m.to(dev).train()
    x, y = _t(g["x"], dev), _t(g["y"], dev)
    out, info = m(x, None, None, None)
    loss = F.cross_entropy(out, y) + info.loss.mean() + F.cross_entropy(info.shapelet_preds, y)
    loss.backward()
    for k, v in (("out", out), ("eta", info.eta), ("shapelet_preds", info.shapelet_preds), ("dnn_preds", info.dnn_preds),
                 ("p", info.p), ("model_loss", info.loss)):
        parity("n39." + k, v, g[k], kind="elem")
    parity("n39.train_loss", loss, g["train_loss"], kind="elem")
    for n, p in m.named_parameters():
        if n.startswith("deep_model.block") and n.endswith(".0.bias"):
            continue
        _compact_close("n39.grad", p.grad, g, "grad", n)
    m.eval()
    with torch.no_grad():
        oe, _ = m(x, None, None, None)
        og, ig = m(x, None, None, None, gating_value=0.05)
    parity("n39.eval_out", oe, g["eval_out"], kind="elem")
    parity("n39.gated_out", og, g["gated_out"], kind="elem")
    parity("n39.gated_eta", ig.eta, g["gated_eta"], kind="elem")


def test_three_adam_steps_n39():
    dev = _dev()
    _lib()
    from models.InterpGN import InterpGN
    g = golden("train_step_ign_n39")
    m = InterpGN(make_cfg(num_class=39, c_out=39))
    m.load_state_dict(_sd32(g, "sd0."))
    m.to(dev).train()
    opt = torch.optim.Adam(m.parameters(), lr=5e-3)
    xs, ys = _t(g["xs"], dev), _t(g["ys"], dev)
    for i in range(3):
        out, info = m(xs[i], None, None, None)
        loss = F.cross_entropy(out, ys[i]) + info.loss.mean() + F.cross_entropy(info.shapelet_preds, ys[i])
        loss.backward()
        opt.step()
        opt.zero_grad()
        parity(f"n39.loss_step{i}", loss, np.float64(g["losses"][i]), kind="elem")
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


# ------------------------------------------------------------------------------------------------------------ launch budget
def _kernel_counts(step, n=3):
    from torch.profiler import ProfilerActivity, profile
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(n):
            step()
        torch.cuda.synchronize()
    names = {}
    for ev in prof.events():
        if str(getattr(ev, "device_type", "")).endswith("CUDA") and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower():
            # template arguments dropped: the chunked and single-pass instantiations of one kernel template are the same kernel,
            # and torch's softmax (the SBM step's cross-entropy) is instantiated per log2 of the row width
            key = ev.name
            while re.search(r"<[^<>]*>", key):
                key = re.sub(r"<[^<>]*>", "", key)
            key = key.replace("ign_loss_wide_kernel", "ign_loss_kernel")     # the loss tail above 16 classes: same role
            names[key] = names.get(key, 0) + 1
    if not names:
        pytest.skip("torch.profiler reported no device events here")
    return {k: v / n for k, v in names.items()}


def _ign_step_counts(N, model_name):
    dev = _dev()
    _lib()
    from ign_hip import ops
    from ign_hip.ddp import FlatAdam, FlatParamBucket
    from models.InterpGN import InterpGN
    from models.Shapelet import ShapeBottleneckModel
    cfg = make_cfg(num_class=N, c_out=N)
    torch.manual_seed(0)
    if model_name == "InterpGN":
        model = InterpGN(cfg).to(dev).train()
    else:
        model = ShapeBottleneckModel(cfg, [5, 5, 5, 5], [0.1, 0.2, 0.3, 0.5]).to(dev).train()
    bucket = FlatParamBucket(model, 1)
    opt = FlatAdam(bucket, lr=5e-3)
    x = torch.randn(32, 100, 6, device=dev)
    y = (torch.arange(32) % N).to(dev)
    mask = torch.ones(32, 100, device=dev)

    def step():
        if model_name == "InterpGN":
            out, info = model(x, mask, None, None)
            loss = ops.ign_loss(info.shapelet_preds, info.dnn_preds, y, 1.0, reg=info.loss)[0]
        else:
            out, info = model(x)
            loss = F.cross_entropy(out, y) + info.loss.mean()
        ops.backward(loss)
        opt.step()
        bucket.zero_grad()

    return _kernel_counts(step)


@pytest.mark.parametrize("model_name", ["InterpGN", "SBM"])
def test_step_at_39_classes_launches_what_the_4_class_step_launches(model_name):
    _dev()
    from ign_hip import fcn
    if fcn.CONV_MATH != "f16x3":
        pytest.skip("the budget is that of the default arithmetic (IGN_CONV_MATH=f16x3)")
    c4 = _ign_step_counts(4, model_name)
    c39 = _ign_step_counts(39, model_name)
    assert sum(c39.values()) == sum(c4.values()) and c39 == c4, f"N=4: {c4}\nN=39: {c39}"


# ------------------------------------------------------------------------------------------------------------ hipGraph
def test_hipgraph_harness_run_at_39_classes_equals_the_eager_run(tmp_path, monkeypatch):
    _dev()
    _lib()
    import run
    from exp.experiment_classification import Experiment
    monkeypatch.chdir(tmp_path)
    outs = {}
    for mode in ("eager", "graph"):
        argv = ["--model", "InterpGN", "--dnn_type", "FCN", "--data", "SYNTH", "--synthetic", "104,6,100,39", "--dataset",
                "g39" + mode, "--batch_size", "32", "--amp", "--train_epochs", "2", "--num_workers", "0", "--seed", "0",
                "--patience", "10"] + (["--hipgraph"] if mode == "graph" else [])
        a = run.get_args(argv)
        run.set_seed(0)
        e = Experiment(a)
        torch.manual_seed(123)
        e.train()
        outs[mode] = {k: v.detach().float().cpu().clone() for k, v in e.model.state_dict().items()}
        if mode == "graph":
            assert getattr(e, "_graphed", None) is not None and e.optimizer.capturable
    for k, v in outs["eager"].items():
        assert torch.equal(v, outs["graph"][k]), k


# ------------------------------------------------------------------------------------------------------------ drivers
def _run_driver(cwd, args):
    r = subprocess.run([sys.executable, os.path.join(PKG, "run.py")] + args, cwd=cwd, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "accuracy:" in r.stdout, r.stdout[-2000:]
    pk = [os.path.join(d, f) for d, _, fs in os.walk(cwd) for f in fs if f == "test_results.pkl"]
    assert pk, r.stdout[-1000:]
    with open(pk[0], "rb") as f:
        res = pickle.load(f)
    assert np.isfinite(res["test_loss"])
    return res


def test_run_py_chisco_39_categories(tmp_path):
    _dev()
    rng = np.random.RandomState(3)
    y = np.concatenate([np.arange(39), rng.randint(0, 39, size=81)])
    X = (rng.randn(120, 6, 100) * 20 + 300).astype(np.float32)
    X[:, 0, 10:30] += (y % 13)[:, None] * 40.0
    np.save(tmp_path / "X.npy", X)
    np.save(tmp_path / "y.npy", y)
    _run_driver(str(tmp_path), ["--model", "InterpGN", "--dnn_type", "FCN", "--data", "EEG", "--data_root", str(tmp_path),
                                "--dataset", "chisco_npy", "--train_epochs", "2", "--batch_size", "32", "--seed", "0", "--amp",
                                "--num_workers", "0"])


def test_run_py_uea_25_classes_hipgraph(tmp_path):
    _dev()
    _lib()
    from data_provider.ts_reader import write_ts
    d = tmp_path / "data" / "Synth25"
    os.makedirs(d)
    classes = [f"c{k}" for k in range(25)]
    tt = np.arange(60)
    for split, seed, n in (("TRAIN", 1, 100), ("TEST", 2, 50)):
        rng = np.random.RandomState(seed)
        X, y = [], []
        for i in range(n):
            k = i % 25
            X.append(rng.randn(3, 60) * 0.5 + np.sin(2 * np.pi * (k + 1) * tt / 60)[None, :])
            y.append(classes[k])
        write_ts(str(d / f"Synth25_{split}.ts"), X, y, "Synth25", classes)
    _run_driver(str(tmp_path), ["--model", "InterpGN", "--dnn_type", "FCN", "--data", "UEA", "--data_root", str(tmp_path / "data"),
                                "--dataset", "Synth25", "--train_epochs", "2", "--batch_size", "32", "--seed", "0", "--amp",
                                "--hipgraph", "--num_workers", "0"])


# ------------------------------------------------------------------------------------------------------------ DNN heads
def test_dnn_fcn_39_classes_vs_oracle():
    dev = _dev()
    _lib()
    from models.FullyConvNet import FullyConvNetwork
    from oracle import ign_oracle as O
    cfg = make_cfg(num_class=39, c_out=39)
    torch.manual_seed(0)
    ref = O.OracleFCN(cfg).train()
    m = FullyConvNetwork(cfg)
    m.load_state_dict(ref.state_dict())
    m.to(dev).train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(16, 100, 6, generator=g)
    y = torch.randperm(39, generator=g)[:16]
    o_r = ref(x)
    F.cross_entropy(o_r, y).backward()
    o = m(x.to(dev))
    F.cross_entropy(o, y.to(dev)).backward()
    parity("fcn39.out", o, o_r.detach(), kind="elem", ref_is="CPU oracle fp32")
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        if n.startswith("block") and n.endswith(".0.bias"):
            continue
        parity(f"fcn39.grad.{n}", p.grad, q.grad, kind="scale", floor=1e-7, ref_is="CPU oracle fp32")


def test_head_linear_39_classes_runs_the_hip_head_vs_float64():
    """ops.head_linear above 16 classes -- the route of the EEG-CNN classifier (models/eegcnn.py) and of the unfused FCN head --
    is HeadLinearFn on the HIP kernels, no longer torch's GEMM."""
    dev = _dev()
    _lib()
    from ign_hip import ops
    torch.manual_seed(1)
    for B, F_ in ((32, 128), (256, 512)):
        x = torch.randn(B, F_, device=dev, requires_grad=True)
        w = torch.randn(39, F_, device=dev, requires_grad=True)
        b = torch.randn(39, device=dev, requires_grad=True)
        out = ops.head_linear(x, w, b)
        assert out.grad_fn is not None and "HeadLinearFn" in type(out.grad_fn).__name__
        go = torch.randn(B, 39, device=dev)
        out.backward(go)
        x64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (x, w, b))
        o64 = x64 @ w64.T + b64
        o64.backward(go.double())
        parity("head_linear39.out", out, o64.detach(), tol=1e-5, kind="scale", ref_is="float64")
        for t, r, n in ((x, x64, "x"), (w, w64, "w"), (b, b64, "b")):
            parity(f"head_linear39.grad_{n}", t.grad, r.grad, tol=1e-5, kind="scale", ref_is="float64")

