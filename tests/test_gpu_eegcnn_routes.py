"""EEG-CNN off its fast window (2 <= k1 <= 125, k1 <= T <= 1024) on an MI355X: every fallback route against float64.

Op level: the rows of tests/eegcnn_route_cases.py -- the generic depthwise kernels dwconv1d_kernel<false> / <true> and
dwconv1d_bwd_w_kernel, autocorr_kernel, EEGcnn._window_gram over them, ign_conv1_sumsq_* at the shapes the model routes to it, the
grid-stride loop and the alignment fallback of ign_chan_contract_bwd_weight, and the switch points of the wave kernel -- each against
float64 torch of the same operation, at the bound the suite already holds the fast-window kernels to.  Every row also asks the
device which side of xcorr_geometry it is on (ign_autocorr_sum_fwd refuses before any launch exactly where the geometry does).

Model level: two training steps and an eval forward of EEGcnn against the layer-by-layer evaluation of a float64 CPU copy, with
every parameter gradient and the whole state_dict; the refusals, which come from forward before anything is launched or updated.

IGN_EEGCNN_ROUTES_OUT=FILE writes the observed errors as JSON (tests/diag_eegcnn_routes.py merges them into
profiles/eegcnn_routes.json)."""
import copy
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

import eegcnn_route_cases as R
from conftest import parity
from test_gpu_baselines import _eegcnn_reference_ops

pytestmark = pytest.mark.gpu
F64 = "float64 torch (CPU)"
_REC = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    out = os.environ.get("IGN_EEGCNN_ROUTES_OUT")
    if out and _REC:
        with open(out, "w") as f:
            json.dump(dict(gpu_rows=_REC), f, indent=1, sort_keys=True)


def _check(table, row, label, got, ref, tol):
    """parity(kind="scale") at `tol`, recorded per table row"""
    rec = parity(f"{row}: {label}", got, ref, tol=tol, kind="scale", ref_is=F64)
    _REC.setdefault(table, {}).setdefault(str(row), {})[label] = dict(error=rec["max_abs_err"] / rec["scale"], bound=tol)
    print(f"{table} {row} {label}: {rec['max_abs_err'] / rec['scale']:.3e} (bound {tol:.0e})")


def _device_side_of_the_switch(table, row, T, K):
    """ign_autocorr_sum_fwd at (T, K): IGN_E_UNSUP exactly where the restatement says xcorr_geometry refuses"""
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    L = _lib.lib()
    dev = _dev()
    x = torch.zeros(1, T, device=dev)
    part = torch.zeros(int(L.ign_autocorr_parts(1)) * K, device=dev)
    rs = torch.zeros(4, device=dev)
    used = ctypes.c_int(-1)
    rc = L.ign_autocorr_sum_fwd(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(part.data_ptr()), ctypes.c_void_p(rs.data_ptr()), 1, T, K,
                                ctypes.byref(used), _lib.stream())
    torch.cuda.synchronize()
    refuses = R.autocorr_sum_refuses(T, K)
    assert rc == (R.E_UNSUP if refuses else 0), f"{row}: ign_autocorr_sum_fwd(T={T}, K={K}) -> {rc}, restatement refuses: {refuses}"
    assert used.value == (-1 if refuses else 1)
    _REC.setdefault(table, {}).setdefault(str(row), {})["xcorr_geometry_accepts"] = not refuses


# ------------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("shape,want,why", R.DWCONV_CASES, ids=[str(c[0]) for c in R.DWCONV_CASES])
def test_dwconv1d_routes_vs_float64(shape, want, why):
    """y, dx (the flipped forward kernel) and dw of ops.dwconv1d against autograd through F.conv1d in float64"""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    B, C, T, k = shape
    route = R.dwconv_route(T, k, B)
    if k <= R.AC_LAGS:
        _device_side_of_the_switch("dwconv1d", shape, T, k)
        assert (route["dw"] == "xcorr_kernel") == (not R.autocorr_sum_refuses(T, k))
    else:
        assert route["dw"] == "dwconv1d_bwd_w_kernel"
    g = torch.Generator().manual_seed(7 * T + k)
    x = torch.randn(B, C, T, generator=g).to(dev).requires_grad_(True)
    w = torch.randn(C, k, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(B, C, T, generator=g)
    pl = (k - 1) // 2
    y = ops.dwconv1d(x, w, pl)
    (y * go.to(dev)).sum().backward()
    xd, wd = x.detach().double().cpu().requires_grad_(True), w.detach().double().cpu().requires_grad_(True)
    yr = F.conv1d(F.pad(xd, (pl, k - 1 - pl)), wd.unsqueeze(1), groups=C)
    (yr * go.double()).sum().backward()
    _REC.setdefault("dwconv1d", {}).setdefault(str(shape), {})["route"] = dict(fwd=route["fwd"], TT=route["TT"], dw=route["dw"])
    _check("dwconv1d", shape, "y", y, yr, R.DW_Y_TOL)
    _check("dwconv1d", shape, "dx", x.grad, xd.grad, R.DW_DX_TOL)
    _check("dwconv1d", shape, "dw", w.grad, wd.grad, R.DW_DW_TOL)


def _lag_sums64(x, K):
    xd = x.double()
    T = xd.shape[1]
    return torch.stack([(xd[:, :T - d] * xd[:, d:]).sum() if d < T else xd.new_zeros(()) for d in range(K)])


@pytest.mark.parametrize("shape,want,why", R.AUTOCORR_CASES, ids=[str(c[0]) for c in R.AUTOCORR_CASES])
def test_autocorr_routes_vs_float64(shape, want, why):
    """ops.autocorr: C[d] = sum_rows sum_u x[u] x[u + d], on autocorr_kernel beyond 1024 samples"""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    Rr, T, K = shape
    _device_side_of_the_switch("autocorr", shape, T, K)
    assert (want["kernel"] == "xcorr_kernel") == (not R.autocorr_sum_refuses(T, K))
    g = torch.Generator().manual_seed(Rr + T + K)
    x = torch.randn(Rr, T, generator=g) + 0.3
    C = ops.autocorr(x.to(dev), K)
    assert C.dtype == torch.float64 and tuple(C.shape) == (K,)
    _REC.setdefault("autocorr", {}).setdefault(str(shape), {})["route"] = want["kernel"]
    _check("autocorr", shape, "C", C, _lag_sums64(x, K), R.LAG_TOL)


@pytest.mark.parametrize("shape,want,why", R.GRAM_CASES, ids=[str(c[0]) for c in R.GRAM_CASES])
def test_window_gram_routes_vs_float64(shape, want, why):
    """EEGcnn._window_gram beyond 1024 samples against the brute-force Gram matrix of all padded windows, and its quadratic form
    against sum_t (w (*) x)^2 of the convolution itself"""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    from models.eegcnn import EEGcnn
    Rr, T, k, pl = shape
    _device_side_of_the_switch("window_gram", shape, T, k)
    assert R.autocorr_sum_refuses(T, k)
    g = torch.Generator().manual_seed(Rr + T + k)
    x = torch.randn(Rr, T, generator=g) + 0.3
    G = EEGcnn._window_gram(x.to(dev), k, pl).cpu()
    xp = F.pad(x.double(), (pl, k - 1 - pl))
    W = xp.unfold(1, k, 1)[:, :T]
    Gref = torch.einsum('rtj,rtk->jk', W, W)
    _REC.setdefault("window_gram", {}).setdefault(str(shape), {})["route"] = f"{want['kernel']} + {want['edges']}"
    _check("window_gram", shape, "G", G, Gref, R.LAG_TOL)
    w = torch.randn(4, k, generator=g).double()
    y = F.conv1d(xp.unsqueeze(1), w.unsqueeze(1))
    _check("window_gram", shape, "w^T G w", torch.einsum('fj,jk,fk->f', w, G, w), y.square().sum(dim=(0, 2)), R.LAG_TOL)


@pytest.mark.parametrize("shape,why", R.SUMSQ_CASES, ids=[str(c[0]) for c in R.SUMSQ_CASES])
def test_conv1_sumsq_routes_vs_float64(shape, why):
    """sum (w1 (*) x - mu)^2 and its gradient at long rows, rows shorter than the kernel and kernels beyond 128 taps"""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    Rr, T, F1, k1 = shape
    g = torch.Generator().manual_seed(Rr * 31 + k1)
    x = (torch.randn(Rr, T, generator=g) * 1.5 + 0.3).to(dev)
    w = (torch.randn(F1, k1, generator=g) * 0.2).to(dev).requires_grad_(True)
    pl = (k1 - 1) // 2
    xd, wd = x.double().cpu(), w.detach().double().cpu().requires_grad_(True)
    y = F.conv1d(F.pad(xd.unsqueeze(1), (pl, k1 - 1 - pl)), wd.unsqueeze(1))
    mu = y.mean(dim=(0, 2))
    m2_ref = ((y - mu.view(1, -1, 1)) ** 2).sum(dim=(0, 2))
    cot = torch.randn(F1, generator=g).double()
    (m2_ref * cot).sum().backward()
    m2 = ops.conv1_sumsq(x, w, mu.detach().float().to(dev), pl)
    (m2 * cot.float().to(dev)).sum().backward()
    _REC.setdefault("conv1_sumsq", {}).setdefault(str(shape), {})["route"] = why
    _check("conv1_sumsq", shape, "m2", m2, m2_ref, R.SUMSQ_TOL)
    _check("conv1_sumsq", shape, "dw1", w.grad, wd.grad, R.SUMSQ_GRAD_TOL)       # (d/dmu = 0 exactly: mu is the batch mean)


@pytest.mark.parametrize("shape,off,want,why", R.CHAN_CASES, ids=[f"{c[0]}+{c[1]}" for c in R.CHAN_CASES])
def test_chan_contract_routes_vs_float64(shape, off, want, why):
    """u, dW and dx of the channel contraction with more slices than blocks; with `off`, x and du are contiguous views that start
    `off` floats into a larger buffer, which sends a T % 4 = 0 shape to the VALU kernel"""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ops
    B, Ci, Co, T = shape
    g = torch.Generator().manual_seed(B + T + off)

    def based(*dims):
        n = 1
        for d in dims:
            n *= d
        buf = torch.zeros(n + 8, device=dev)
        v = buf[off:off + n].view(*dims)
        v.copy_(torch.randn(*dims, generator=g))
        assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
        return v

    x, du = based(B, Ci, T), based(B, Co, T)
    w = torch.randn(Co, Ci, generator=g).to(dev)
    assert R.cw_plan(B, T, aligned=x.data_ptr() % 16 == 0 and du.data_ptr() % 16 == 0) == R.cw_plan(B, T, aligned=off == 0)
    L = _lib.lib()
    u = ops.ChanContractFn._run(x, w)
    dx = ops.ChanContractFn._run(du, w.t().contiguous())
    ws = torch.empty(L.ign_chan_contract_bwd_weight_workspace_bytes(B, Ci, Co, T) // 4, device=dev)
    assert ws.numel() == want["blocks"] * Co * Ci
    dw = torch.empty(Co, Ci, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(L.ign_chan_contract_bwd_weight(p(du), p(x), p(dw), p(ws), B, Ci, Co, T, _lib.stream()), "ign_chan_contract_bwd_weight")
    xd, dud, wd = x.double().cpu(), du.double().cpu(), w.double().cpu()
    row = f"{shape}+{off}"
    _REC.setdefault("chan_contract", {}).setdefault(row, {})["route"] = want["kernel"] + (", grid-stride" if want["grid_stride"] else "")
    _check("chan_contract", row, "u", u, torch.einsum('oc,bct->bot', wd, xd), R.CC_TOL)
    _check("chan_contract", row, "dW", dw, torch.einsum('bot,bct->oc', dud, xd), R.CC_TOL)
    _check("chan_contract", row, "dx", dx, torch.einsum('oc,bot->bct', wd, dud), R.CC_TOL)
    if off == 0:
        # the same through autograd: the route the model takes
        xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        (ops.chan_contract(xg, wg) * du).sum().backward()
        assert torch.equal(wg.grad, dw) and torch.equal(xg.grad, dx)


# ------------------------------------------------------------------------------------------------------------- model level
def _model(shape, dev):
    import speech_imagery_eeg_amd  # noqa: F401
    from models.eegcnn import EEGcnn
    B, C, T, k1, k2, F1, D, P1, P2 = shape
    torch.manual_seed(T + k1 + 1)
    m = EEGcnn(Chans=C, kernLength1=k1, kernLength2=k2, F1=F1, D=D, F2=F1 * D, P1=P1, P2=P2, dropoutRate=0.0)
    with torch.no_grad():
        for bn in (m.block1_bn1, m.block1_bn2, m.block2_bn):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
    return m


def _state(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("case", R.MODEL_CASES, ids=[c[0] for c in R.MODEL_CASES])
def test_eegcnn_routes_two_steps_and_eval_vs_float64(case, monkeypatch):
    """Two training steps (running statistics updated twice, parameters moved in between) and an eval forward against the
    layer-by-layer evaluation of a float64 CPU copy: outputs, every parameter gradient of the first step, the whole state_dict."""
    name, shape, opts, route, why = case
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    from models import eegcnn
    B, C, T = shape[:3]
    m = _model(shape, dev)
    if "variance_switch" in opts:
        monkeypatch.setattr(eegcnn, "_BN1_VARIANCE", opts["variance_switch"])
    if "momentum" in opts:
        m.block1_bn1.momentum = opts["momentum"]
    ref = copy.deepcopy(m).double()
    m.to(dev)
    g = torch.Generator().manual_seed(B + T)
    xs = [torch.randn(B, C, T, generator=g) * 1.5 + 0.2 for _ in range(3)]
    _REC.setdefault("model", {}).setdefault(name, {})["route"] = route
    m.train(); ref.train()
    for step in (1, 2):
        a, b = m(xs[step - 1].to(dev)), _eegcnn_reference_ops(ref, xs[step - 1].double())
        assert torch.isfinite(a).all()
        _check("model", name, f"out step {step}", a, b, R.MODEL_TOL)
        ga = torch.autograd.grad(a.square().sum(), list(m.parameters()), allow_unused=True)
        gb = torch.autograd.grad(b.square().sum(), list(ref.parameters()))
        if step == 1:
            top = float(max(t.abs().max() for t in gb))
            for (n, _), u, v in zip(m.named_parameters(), ga, gb):
                if n in R.zero_grad_params(shape[3]):
                    # removed by the next BatchNorm: the true gradient is below 1e-4 of the largest, and so must the HIP one be
                    assert float(v.abs().max()) < 1e-4 * top, n
                    assert u is None or float(u.abs().max()) < 1e-4 * top, (n, float(u.abs().max()), top)
                    continue
                assert u is not None and torch.isfinite(u).all(), n
                _check("model", name, "grad." + n, u, v, R.MODEL_TOL)
            with torch.no_grad():           # move every parameter (the same move on both sides) before the second step
                for p, q, v in zip(m.parameters(), ref.parameters(), gb):
                    q.sub_(0.05 * v / v.abs().max().clamp_min(1e-30))
                    p.copy_(q.float())
    m.eval(); ref.eval()
    with torch.no_grad():
        _check("model", name, "out eval", m(xs[2].to(dev)), _eegcnn_reference_ops(ref, xs[2].double()), R.MODEL_TOL)
    sd, sdr = m.state_dict(), ref.state_dict()
    assert list(sd) == list(sdr)
    for k in sd:
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(sdr[k]) == 2, k
        _check("model", name, "sd." + k, sd[k].float(), sdr[k].double(), R.MODEL_TOL)


def _assert_refused_untouched(m, x, match):
    from ign_hip._lib import IgnError
    before = _state(m)
    with pytest.raises(IgnError, match=match):
        m(x)
    torch.cuda.synchronize()
    after = m.state_dict()
    for k, v in before.items():
        assert torch.equal(v, after[k]), f"{k} changed by a refused forward"
    assert int(m.block1_bn1.num_batches_tracked) == 0


def test_kernel_beyond_128_taps_at_eight_filters_is_refused_by_forward():
    """k1 = 131 at F1 = 8 has no BatchNorm-1 variance gradient: forward says so, naming the limit, before anything moves (it used
    to arrive from the middle of backward(), after the running statistics of the step had been written)"""
    dev = _dev()
    B, C, T, k1 = R.REFUSED_TAPS["shape"][:4]
    m = _model(R.REFUSED_TAPS["shape"], dev).to(dev).train()
    x = torch.randn(B, C, T, device=dev)
    _assert_refused_untouched(m, x, rf"k1 <= {R.conv1_sumsq_max_taps(8)}\b")
    m.eval()
    with torch.no_grad():
        assert torch.isfinite(m(x)).all()             # running statistics: nothing to refuse


def test_row_beyond_the_lds_tiles_is_refused_by_forward():
    dev = _dev()
    B, C, T, k1 = R.REFUSED_ROW["shape"][:4]
    m = _model(R.REFUSED_ROW["shape"], dev).to(dev).train()
    _assert_refused_untouched(m, torch.randn(B, C, T, device=dev), rf"T \+ k1 <= {R.ROW_TILE_MAX}\b")
    m.eval()
    _assert_refused_untouched(m, torch.randn(B, C, T, device=dev), rf"T \+ k1 <= {R.ROW_TILE_MAX}\b")
