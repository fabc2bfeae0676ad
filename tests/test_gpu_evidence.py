"""Evidence maps on the GPU: ign_shapelet_evidence_bank and ign_cam_spread against the numpy restatement of csrc/ign_evidence.h
(utils/evidence.py) bit for bit, ign_bn_relu_cam_fwd against float64 of the same fp32 operands, and utils.evidence.evidence_map end to
end through SBM, LTS, InterpGN + FCN and a bare FCN.  The host side (the rule against a triple loop, refusals, the flag) is
tests/test_evidence_host.py; the cases are tests/evidence_cases.py.

Bounds (none is measured; U = 2^-24).
  cam: a term is W * relu(fma(a, y, b)) -- two roundings -- summed over Cl channels in some order (at most Cl - 1 roundings deep),
    times fl(1/Tl) (two more): |cam - exact| <= (Cl + 3) U (1/Tl) sum_c |W| |h|.  The scaled map is fl(cam * scale) to the bit.
  completeness: the maps are fp32 shares of a logit the forward summed in another order; the float64 sum of the n non-zero shares
    differs from that logit by at most (n + 3) U sum |shares| (evidence_cases.sum_bound).
  float64 parity of cam through the whole FCN: the project's 1e-4 budget relative to max |cam| (conftest.parity)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from conftest import make_cfg, parity
from evidence_cases import BANK, BANK_WIDE, CLASSES, SHAPES, U, make_case, same_bits, sum_bound

pytestmark = pytest.mark.gpu
GUARD = 1024


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _mods():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ops
    from utils import evidence
    return _lib, ops, evidence


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------- evidence kernel
def _run_bank(dev, case, N):
    """One launch of the entry point into a NaN-filled buffer with GUARD sentinel floats behind it -> (out (B,T,C), guard)."""
    _lib, _, _ = _mods()
    B, ld = case["p"].shape
    T, C, G = case["T"], case["C"], len(case["Ks"])
    p, W = torch.from_numpy(case["p"]).to(dev), torch.from_numpy(case["W"]).to(dev)
    t, tg = torch.from_numpy(case["t"]).to(dev), torch.from_numpy(case["target"].astype(np.int32)).to(dev)
    sc = torch.from_numpy(case["scale"]).to(dev) if case["scale"] is not None else None
    n = B * T * C
    buf = torch.full((n + GUARD,), float("nan"), device=dev)
    buf[n:] = 12345.0
    ints, floats = ctypes.c_int * G, ctypes.c_float * G
    col0s = [sum(k * C for k in case["Ks"][:g]) for g in range(G)]
    invL = [float(np.float32(1.0) / np.float32(v)) for v in case["Ls"]]
    _lib.check(_lib.lib().ign_shapelet_evidence_bank(_p(p), _p(t), _p(W), _p(tg), _p(sc), ld, G, ints(*case["Ks"]), ints(*case["Ls"]),
                                                     ints(*case["strides"]), ints(*col0s), floats(*invL), _p(buf), B, T, C, N, _s()),
               "ign_shapelet_evidence_bank")
    torch.cuda.synchronize()
    return buf[:n].view(B, T, C).cpu().numpy(), buf[n:].cpu().numpy()


def _rule(evidence, case):
    return evidence.evidence_rule(case["p"], case["t"], case["W"], case["target"], case["Ks"], case["Ls"], case["strides"], case["C"],
                                  case["T"], case["scale"])


@pytest.mark.parametrize("N", CLASSES)
@pytest.mark.parametrize("scale", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_evidence_kernel_equals_the_rule_bit_for_bit(shape, scale, N):
    dev = _dev()
    _, _, evidence = _mods()
    B, T, C = shape
    case = make_case(B, T, C, N, seed=B + T + C + N, scale=scale, **BANK)
    assert (case["t"] == -1).any() and len(set(case["target"].tolist())) > 1
    got, guard = _run_bank(dev, case, N)
    ref = _rule(evidence, case)
    assert same_bits(got, ref), f"max |diff| {np.nanmax(np.abs(got - ref))}, NaNs left {int(np.isnan(got).sum())}"
    assert (guard == 12345.0).all()
    again, _ = _run_bank(dev, case, N)
    assert same_bits(got, again)


@pytest.mark.parametrize("shape", [(2, 37, 3), (2, 64, 65)], ids=str)
def test_evidence_kernel_many_shapelets_runs_the_chunk_loop(shape):
    """sum K = 530: more terms than one LDS chunk holds at 4 electrode lanes (512 features) and at 128 (16 features)"""
    dev = _dev()
    _, _, evidence = _mods()
    B, T, C = shape
    case = make_case(B, T, C, 3, seed=7, scale=True, **BANK_WIDE)
    got, guard = _run_bank(dev, case, 3)
    assert same_bits(got, _rule(evidence, case)) and (guard == 12345.0).all()


def test_uncovered_positions_are_exactly_zero_and_the_op_checks_its_arguments():
    dev = _dev()
    _lib, ops, evidence = _mods()
    B, T, C, N = 3, 37, 5, 3
    case = make_case(B, T, C, N, seed=3, **BANK)
    only = np.full_like(case["t"], -1)
    only[:, 1] = 30                                  # group 0 (L = 4), shapelet 0, electrode 1: samples 30..33
    case["t"] = only
    got, _ = _run_bank(dev, case, N)
    assert (got[:, 30:34, 1] != 0).all() and np.count_nonzero(got) == B * 4 and not np.isnan(got).any()
    assert same_bits(got, _rule(evidence, case))
    # through ops: the same bits; refusals come before the launch
    case = make_case(B, T, C, N, seed=4, scale=True, **BANK)
    args = [torch.from_numpy(case[k]).to(dev) for k in ("p", "t", "W", "target")]
    sc = torch.from_numpy(case["scale"]).to(dev)
    out = ops.shapelet_evidence(*args, case["Ks"], case["Ls"], case["strides"], C, T, scale=sc)
    assert same_bits(out.cpu().numpy(), _rule(evidence, case))
    bad_t = args[1].clone()
    bad_t[1, 0] = T
    with pytest.raises(_lib.IgnError, match="match location outside"):
        ops.shapelet_evidence(args[0], bad_t, args[2], args[3], case["Ks"], case["Ls"], case["strides"], C, T)
    with pytest.raises(_lib.IgnError, match="target outside"):
        ops.shapelet_evidence(args[0], args[1], args[2], args[3] + N, case["Ks"], case["Ls"], case["strides"], C, T)
    with pytest.raises(_lib.IgnError, match="p, t must be"):
        ops.shapelet_evidence(args[0][:, :-1], args[1][:, :-1], args[2], args[3], case["Ks"], case["Ls"], case["strides"], C, T)
    with pytest.raises(_lib.IgnError, match="int32"):
        ops.shapelet_evidence(args[0], args[1].long(), args[2], args[3], case["Ks"], case["Ls"], case["strides"], C, T)
    with pytest.raises(_lib.IgnError, match="no CPU fallback"):
        ops.shapelet_evidence(args[0].cpu(), args[1], args[2], args[3], case["Ks"], case["Ls"], case["strides"], C, T)


# ------------------------------------------------------------------------------------------------------------- CAM kernel
# the issue's three, plus the other routes of the kernel: a row wider than a wave's 64 quads (coefficients re-read per step), and a
# quad count that is no power of two (an idle lane inside a row's lane group)
CAM_SHAPES = [(2, 1, 4), (2, 67, 128), (1, 130, 256), (1, 3, 1024), (3, 70, 12)]


def _cam_inputs(B, Tl, Cl, N, negative=False):
    g = torch.Generator().manual_seed(B + Tl + Cl + N)
    y = torch.randn(B, Tl, Cl, generator=g)
    a = torch.randn(Cl, generator=g)
    b = torch.randn(Cl, generator=g) * 0.5
    if negative:                                    # every pre-activation negative
        y, a, b = y.abs() + 0.1, -a.abs() - 0.1, -b.abs()
    W = torch.randn(N, Cl, generator=g)
    target = (torch.arange(B) * 2 + 1) % N
    scale = torch.rand(B, generator=g) + 0.25
    return y, a, b, W, target, scale


@pytest.mark.parametrize("N", CLASSES)
@pytest.mark.parametrize("shape", CAM_SHAPES, ids=str)
def test_cam_kernel_against_float64(shape, N):
    dev = _dev()
    _, ops, _ = _mods()
    B, Tl, Cl = shape
    y, a, b, W, target, scale = _cam_inputs(B, Tl, Cl, N)
    cam = ops.fcn_cam(y.to(dev), a.to(dev), b.to(dev), W.to(dev), target.to(dev))
    assert cam.shape == (B, Tl) and cam.dtype == torch.float32
    h = torch.relu(a.double() * y.double() + b.double())
    terms = W.double()[target][:, None, :] * h                                   # (B,Tl,Cl)
    ref = terms.sum(-1) / Tl
    bound = (Cl + 3) * U * terms.abs().sum(-1) / Tl
    err = (cam.cpu().double() - ref).abs()
    print(f"cam {shape} N={N}: worst error / bound = {float((err / bound.clamp_min(1e-300)).max()):.4f}")
    assert bool((err <= bound).all()), f"{float((err / bound).max())} x the bound"
    # the per-sample scale multiplies once, at the end; two runs agree to the bit
    scaled = ops.fcn_cam(y.to(dev), a.to(dev), b.to(dev), W.to(dev), target.to(dev), scale=scale.to(dev))
    assert same_bits(scaled.cpu().numpy(), (cam.cpu() * scale[:, None]).numpy())
    assert same_bits(ops.fcn_cam(y.to(dev), a.to(dev), b.to(dev), W.to(dev), target.to(dev)).cpu().numpy(), cam.cpu().numpy())


def test_cam_is_exactly_zero_where_every_preactivation_is_negative():
    dev = _dev()
    _lib, ops, _ = _mods()
    y, a, b, W, target, scale = _cam_inputs(2, 67, 128, 3, negative=True)
    assert float((a * y + b).max()) < 0
    for sc in (None, scale.to(dev)):
        cam = ops.fcn_cam(y.to(dev), a.to(dev), b.to(dev), W.to(dev), target.to(dev), scale=sc)
        assert bool((cam == 0).all())
    with pytest.raises(_lib.IgnError, match="Cl % 4"):
        ops.fcn_cam(y[:, :, :126].contiguous().to(dev), a[:126].to(dev), b[:126].to(dev), W[:, :126].contiguous().to(dev), target.to(dev))
    with pytest.raises(_lib.IgnError, match="target outside"):
        ops.fcn_cam(y.to(dev), a.to(dev), b.to(dev), W.to(dev), (target + 3).to(dev))


@pytest.mark.parametrize("R", [6, 14])
def test_cam_spread_equals_the_rule_bit_for_bit(R):
    dev = _dev()
    _, ops, evidence = _mods()
    rng = np.random.default_rng(R)
    for Tl in (1, 2, R - 1, R, 67):
        cam = rng.standard_normal((3, Tl)).astype(np.float32)
        out = ops.cam_spread(torch.from_numpy(cam).to(dev), R)
        assert out.shape == (3, Tl + R - 1)
        assert same_bits(out.cpu().numpy(), evidence.cam_spread_rule(cam, R)), (R, Tl)


# ------------------------------------------------------------------------------------------------------------- end to end
B_, T_, C_, N_ = 4, 100, 6, 4


def _x(dev, seed=1):
    return torch.randn(B_, T_, C_, generator=torch.Generator().manual_seed(seed)).to(dev)


def _model(name, dev, seed=0, **kw):
    _mods()
    from models.FullyConvNet import FullyConvNetwork
    from models.InterpGN import InterpGN
    from models.Shapelet import DistThresholdSBM, ShapeBottleneckModel
    torch.manual_seed(seed)
    cfg = make_cfg(enc_in=C_, seq_len=T_, num_class=N_, **kw)
    model = dict(SBM=ShapeBottleneckModel, LTS=DistThresholdSBM, InterpGN=InterpGN, FCN=FullyConvNetwork)[name](cfg)
    for m in model.modules():                       # running statistics that are not the initial (0, 1)
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_(0, 0.3)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.3)
    return model.to(dev).eval()


def _check_complete(ev, label):
    """per sample: the float64 sum of the shares against the model's own logit, within the a-priori bound over the non-zero shares"""
    worst = 0.0
    for b in range(ev.logit.shape[0]):
        parts = [f[b].double().cpu().numpy().ravel() for f in (ev.sbm, ev.dnn) if f is not None]
        if ev.remainder is not None:
            parts.append(np.array([float(ev.remainder[b])]))
        terms = np.concatenate(parts)
        terms = terms[terms != 0]
        bound = sum_bound(terms)
        err = abs(terms.sum() - float(ev.logit[b]))
        worst = max(worst, err / max(bound, 1e-300))
        assert err <= bound, f"{label} sample {b}: |sum - logit| = {err} > {bound}"
    print(f"completeness {label}: worst error / bound = {worst:.4f}")


@pytest.mark.parametrize("name,explain", [("SBM", "sbm"), ("LTS", "sbm"), ("InterpGN", "sbm"), ("InterpGN", "gated"),
                                          ("InterpGN", "dnn"), ("FCN", "dnn")])
def test_maps_sum_to_the_models_own_logit(name, explain):
    dev = _dev()
    _, _, evidence = _mods()
    model, x = _model(name, dev), _x(dev)
    ev = evidence.evidence_map(model, x, explain=explain)
    with torch.no_grad():
        plain = model(x)
    logits = plain if name == "FCN" else plain[0] if explain == "gated" or name != "InterpGN" else \
        (plain[1].shapelet_preds if explain == "sbm" else plain[1].dnn_preds)
    assert torch.equal(ev.target, logits.argmax(1)) and ev.target.dtype == torch.long
    assert torch.equal(ev.logit, logits.gather(1, ev.target[:, None]).squeeze(1))
    has_sbm, has_dnn = explain != "dnn", explain != "sbm"
    assert (ev.sbm is not None) == has_sbm and (ev.contrib is not None) == has_sbm
    assert (ev.dnn is not None) == has_dnn and (ev.cam is not None) == has_dnn and (ev.remainder is not None) == has_dnn
    assert (ev.eta is not None) == (explain == "gated")
    if has_sbm:
        assert ev.sbm.shape == (B_, T_, C_)
        info = plain[1]
        sbm = model.sbm if name == "InterpGN" else model
        assert torch.equal(ev.contrib, sbm.output_layer.weight.detach()[ev.target] * info.p)     # W[target] * p of a plain forward
    if has_dnn:
        assert ev.dnn.shape == (B_, T_) and ev.cam.shape == (B_, T_ - 13) and ev.remainder.shape == (B_,)
    _check_complete(ev, f"{name}/{explain}")
    # a fixed class for the whole batch, and one per sample
    ev2 = evidence.evidence_map(model, x, target=2, explain=explain)
    assert ev2.target.tolist() == [2] * B_
    _check_complete(ev2, f"{name}/{explain}/target=2")
    per = torch.tensor([0, 1, 2, 3])
    assert evidence.evidence_map(model, x, target=per, explain=explain).target.tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="target"):
        evidence.evidence_map(model, x, target=N_, explain=explain)


def test_gated_snaps_to_the_interpretable_expert():
    dev = _dev()
    _, _, evidence = _mods()
    model, x = _model("InterpGN", dev), _x(dev)
    free = evidence.evidence_map(model, x, explain="gated")
    eta = free.eta.cpu()
    gv = float((eta.max() + eta.topk(2).values[1]) / 2)            # only the largest eta exceeds it
    ev = evidence.evidence_map(model, x, explain="gated", gating_value=gv)
    snapped = ev.eta == 1
    assert int(snapped.sum()) == 1 and bool(snapped.cpu()[eta.argmax()])
    assert bool((ev.dnn[snapped] == 0).all()) and bool((ev.cam[snapped] == 0).all()) and bool((ev.remainder[snapped] == 0).all())
    assert bool((ev.dnn[~snapped] != 0).any())
    with torch.no_grad():
        out, info = model(x, None, None, None, gating_value=gv)
    assert torch.equal(ev.eta, info.eta.reshape(-1)) and torch.equal(ev.logit, out.gather(1, ev.target[:, None]).squeeze(1))
    _check_complete(ev, "InterpGN/gated/snapped")
    # the scale went into the kernels: the gated maps are the experts' own maps times eta and 1 - eta, each rounded once
    s = evidence.evidence_map(model, x, target=ev.target, explain="sbm")
    d = evidence.evidence_map(model, x, target=ev.target, explain="dnn")
    assert torch.equal(ev.sbm, s.sbm * ev.eta[:, None, None]) and torch.equal(ev.cam, d.cam * (1.0 - ev.eta)[:, None])


@pytest.mark.parametrize("dist", ["cosine", "pearson"])
def test_cosine_and_pearson_models_return_maps(dist):
    """the distances gradient saliency refuses"""
    dev = _dev()
    _, _, evidence = _mods()
    model, x = _model("SBM", dev, distance_func=dist), _x(dev)
    ev = evidence.evidence_map(model, x)
    assert bool(torch.isfinite(ev.sbm).all()) and bool((ev.sbm != 0).any())
    _check_complete(ev, f"SBM/{dist}")


def test_ragged_batch_under_mask_padding():
    dev = _dev()
    _, _, evidence = _mods()
    model = _model("SBM", dev, mask_padding=True)
    assert [s.length for s in model.shapelets] == [10, 20, 30, 50]
    lengths = [100, 40, 73, 100]                                     # sample 1 is shorter than the longest shapelet
    mask = (torch.arange(T_)[None, :] < torch.tensor(lengths)[:, None]).float().to(dev)
    x = _x(dev) * mask[:, :, None]
    ev = evidence.evidence_map(model, x, mask=mask)
    with torch.no_grad():
        out, info = model(x, mask)
    assert bool((info.t[1] == -1).any()) and not bool((info.t[0] == -1).any())
    assert torch.equal(ev.logit, out.gather(1, ev.target[:, None]).squeeze(1))
    for b, n in enumerate(lengths):
        assert bool((ev.sbm[b, n:] == 0).all()), f"sample {b} painted behind its length {n}"
        assert bool((ev.sbm[b, :n] != 0).any())
    _check_complete(ev, "SBM/mask_padding")


def test_refusals_and_side_effects():
    dev = _dev()
    _, _, evidence = _mods()
    x = _x(dev)
    for cls in ("bilinear", "attention"):
        with pytest.raises(ValueError, match="not additive"):
            evidence.evidence_map(_model("SBM", dev, sbm_cls=cls), x)
    with pytest.raises(TypeError, match="FCN is the supported deep expert"):
        evidence.evidence_map(_model("InterpGN", dev, dnn_type="ResNet"), x, explain="dnn")
    model = _model("InterpGN", dev)
    model.train()
    model.deep_model.block2.eval()                                   # a mixed set-up comes back as it was
    flags = [m.training for m in model.modules()]
    fcn = model.deep_model
    with torch.autocast("cuda", dtype=torch.bfloat16):               # disabled inside the call
        ev = evidence.evidence_map(model, x, explain="gated")
    assert ev.sbm.dtype == ev.dnn.dtype == ev.logit.dtype == torch.float32
    assert [m.training for m in model.modules()] == flags
    assert "keep_last" not in vars(fcn) and fcn.keep_last is False and "last_block" not in vars(fcn)
    assert all(p.grad is None for p in model.parameters())
    fcn.keep_last = True                                             # a switch the user had set stays set, and keeps working
    evidence.evidence_map(model, x, explain="dnn")
    assert fcn.keep_last is True
    model.eval()
    with torch.no_grad():
        fcn(x)
    y_last, a, b = fcn.last_block
    assert y_last.shape == (B_, T_ - 13, 128) and a.shape == b.shape == (128,)
    del fcn.keep_last, fcn.last_block
    with torch.no_grad():
        fcn(x)
    assert not hasattr(fcn, "last_block")                            # off: nothing is kept


def test_cam_float64_parity_through_the_fcn():
    """cam of the HIP forward (eval mode) against a float64 torch FCN on the same weights: 1e-4 of max |cam|"""
    dev = _dev()
    _, _, evidence = _mods()
    model, x = _model("FCN", dev, seed=3), _x(dev, seed=5)
    ev = evidence.evidence_map(model, x, explain="dnn")
    ref = copy.deepcopy(model).double().cpu().eval()
    with torch.no_grad():
        h = ref.block3(ref.block2(ref.block1(x.double().cpu().permute(0, 2, 1))))             # (B,128,Tl)
        logits = ref.fc(h.mean(-1))
        cam = torch.einsum("bct,bc->bt", h, ref.fc.weight[ev.target.cpu()]) / h.shape[-1]
    rec = parity("evidence cam vs float64 FCN", ev.cam, cam, tol=1e-4, kind="scale", ref_is="float64 torch FCN")
    print(f"cam float64 parity: max abs err {rec['max_abs_err']:.3e} at scale {rec['scale']:.3e} = {rec['err_over_1e4']:.4f} x 1e-4")
    parity("evidence dnn logit vs float64 FCN", ev.dnn.sum(1) + ev.remainder, logits.gather(1, ev.target.cpu()[:, None]).squeeze(1),
           tol=1e-4, kind="scale", ref_is="float64 torch FCN")


# ------------------------------------------------------------------------------------------------------------- driver
def test_driver_writes_evidence_npz(tmp_path, capsys, monkeypatch):
    """run.py --evidence gated on the synthetic provider (InterpGN + FCN, one epoch): evidence.npz beside the test results holds the
    maps of the whole test set, and they sum to the logits in it; without the flag no file is written."""
    import glob
    import os
    _dev()
    _mods()
    import run
    monkeypatch.chdir(tmp_path)
    argv = ["--data", "SYNTH", "--synthetic", "24,6,100,4", "--model", "InterpGN", "--dnn_type", "FCN", "--train_epochs", "1",
            "--batch_size", "8", "--seed", "0", "--amp", "--log_interval", "1", "--gating_value", "0.5"]
    run.main(argv + ["--dataset", "plain"])
    assert not glob.glob(str(tmp_path / "checkpoints" / "**" / "evidence.npz"), recursive=True)
    run.main(argv + ["--dataset", "ev", "--evidence", "gated"])
    out = capsys.readouterr().out
    files = glob.glob(str(tmp_path / "checkpoints" / "**" / "evidence.npz"), recursive=True)
    assert len(files) == 1 and "evidence (gated):" in out, out[-2000:]
    assert os.path.exists(os.path.join(os.path.dirname(files[0]), "test_results.pkl"))
    z = dict(np.load(files[0]))
    n = z["logit"].shape[0]
    assert set(z) == {"sbm", "dnn", "cam", "eta", "remainder", "logit", "target", "contrib"} and n > 0
    assert z["sbm"].shape == (n, 100, 6) and z["dnn"].shape == (n, 100) and z["cam"].shape == (n, 87) and z["contrib"].shape == (n, 120)
    assert ((z["eta"] == 1) | (z["eta"] <= 0.5)).all()                                  # --gating_value applied, as in test
    for b in range(n):
        terms = np.concatenate([z["sbm"][b].ravel(), z["dnn"][b], z["remainder"][b:b + 1]]).astype(np.float64)
        terms = terms[terms != 0]
        assert abs(terms.sum() - float(z["logit"][b])) <= sum_bound(terms), b
