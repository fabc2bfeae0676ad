"""GPU parity of the gradient w.r.t. the INPUT series through the shapelet expert: ign_shapelet_bwd_input(_bank),
ign_instnorm_bwd, their autograd nodes in ign_hip.ops, the differentiable SBM / LTS models and utils.saliency.input_saliency,
against fixtures from the reference's autograd (tests/golden/make_golden_input_grad.py) and the CPU oracle's autograd in
float64 on seeded inputs.  Every comparison goes through conftest.parity with kind="scale", tol=1e-4 -- the rule
test_gpu_shapelet.py uses for grad_w (entries are sums of O(K*L) signed terms).  Random cases first assert, on the CPU, that no
input sample is bit-equal to a weight of its channel: at such a tie the kernel's documented sign(0) = -1 differs from aten::sgn."""
import numpy as np
import pytest
import torch

from conftest import golden, make_cfg, parity, sd_from

pytestmark = pytest.mark.gpu

L1, MSE, COS, PEARSON = 0, 1, 2, 3
RBF, LTS = 0x00, 0x10


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _t(a, dev=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev) if dev is not None else t


def _grad_close(label, got, ref):
    parity(label, got, ref, tol=1e-4, kind="scale", floor=1e-12)


def _assert_no_ties(xn, ws, strides=None):
    """the condition on the inputs: no sample x[b,c,s] is bit-equal to a weight w[k,c,j] it meets (s = t*stride + j for a window t)"""
    x = xn.detach().cpu().numpy()
    T = x.shape[2]
    for g, w in enumerate(ws):
        wn = w.detach().cpu().numpy()
        L, stride = wn.shape[2], (strides[g] if strides else 1)
        Tw = (T - L) // stride + 1
        for c in range(x.shape[1]):
            for v in np.intersect1d(x[:, c, :].ravel(), wn[:, c, :].ravel()):
                for s in np.nonzero(x[:, c, :] == v)[1]:
                    for j in np.nonzero(wn[:, c, :] == v)[1]:
                        met = s >= j and (s - j) % stride == 0 and (s - j) // stride < Tw
                        assert not met, f"exact tie: channel {c}, sample {s}, shapelet position {j} of group {g}"


def _oracle_bank(xn, ws, thrs, eps, dist, gate, strides, r, dtype=torch.float64):
    """autograd of sum(P * r) through the oracle (float64 unless told otherwise): -> (P, grad_xn, [grad_w], [grad_thr])"""
    from oracle import ign_oracle as O
    x = xn.detach().cpu().to(dtype).requires_grad_(True)
    w64 = [w.detach().cpu().to(dtype).requires_grad_(True) for w in ws]
    t64 = [t.detach().cpu().to(dtype).requires_grad_(True) for t in thrs] if gate == LTS else []
    ps = []
    for g, w in enumerate(w64):
        d = O.window_distance(x, w, strides[g], O.MODE_L1 if dist == L1 else O.MODE_MSE, chunk=64)
        ps.append(O.lts_softmin_gate(d, t64[g])[0] if gate == LTS else O.rbf_straight_through_max(d, eps)[0])
    P = torch.cat(ps, dim=1)
    grads = torch.autograd.grad((P * r.detach().cpu().to(dtype)).sum(), [x] + w64 + t64)
    G = len(ws)
    return P.detach(), grads[0], list(grads[1:1 + G]), list(grads[1 + G:])


def _hip_bank(dev, xn, ws, thrs, eps, dist, gate, strides, r, x_grad=True):
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    x = xn.to(dev).requires_grad_(x_grad)
    wd = [w.to(dev).requires_grad_(True) for w in ws]
    td = [t.to(dev).requires_grad_(True) for t in thrs] if gate == LTS else None
    P, _ = ops.shapelet_bank(x, wd, eps, dist | gate, list(strides), td)
    (P * r.to(dev)).sum().backward()
    return P.detach(), x.grad, [w.grad for w in wd], [t.grad for t in (td or [])]


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name,mode", [("l1", L1 | RBF), ("mse", MSE | RBF), ("lts", L1 | LTS)])
def test_group_input_grad_matches_the_reference(name, mode):
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    g = golden(f"input_grad_{name}")
    xn = _t(g["xn"], dev).requires_grad_(True)
    w = _t(g["w"], dev).requires_grad_(True)
    thr = [_t(g["thr"], dev)] if "thr" in g else None
    p, _ = ops.shapelet_bank(xn, [w], float(g["eps"]), mode, [1], thr)
    (p * _t(g["r"], dev)).sum().backward()
    parity(f"{name} p", p, g["p"], tol=1e-4, kind="elem")
    assert xn.grad is not None and xn.grad.shape == xn.shape
    _grad_close(f"{name} grad_xn", xn.grad, g["grad_xn"])
    _grad_close(f"{name} grad_w", w.grad, g["grad_w"])


def _sbm_from_fixture(g, head, dev, lts=False):
    import speech_imagery_eeg_amd  # noqa
    from models.Shapelet import ShapeBottleneckModel
    x = _t(g[f"{head}.x"])
    B, T, C = x.shape
    n = int(g[f"{head}.num_shapelet"])
    m = ShapeBottleneckModel(make_cfg(enc_in=C, seq_len=T, num_class=3, c_out=3, dec_in=C, sbm_cls=head),
                             num_shapelet=[n] * 4, shapelet_len=[0.1, 0.2, 0.3, 0.5])
    m.load_state_dict(sd_from(g, prefix=f"{head}.sd."))
    return m.to(dev).eval(), x


@pytest.mark.parametrize("head,fused", [("linear", True), ("linear", False), ("bilinear", True)])
def test_sbm_input_grad_matches_the_reference(head, fused):
    """x.grad of out.sum() through the whole ShapeBottleneckModel (instance norm, bank, head), on the one-node route
    (_fused_forward) and on the route of separate autograd nodes"""
    dev = _dev()
    g = golden("sbm_input_grad")
    m, x = _sbm_from_fixture(g, head, dev)
    if not fused:
        m._fused_forward = lambda x, xn: None
    xd = x.to(dev).requires_grad_(True)
    out, info = m(xd)
    out.sum().backward()
    parity(f"{head} out", out, g[f"{head}.out"], tol=1e-4, kind="elem")
    assert xd.grad is not None and xd.grad.shape == x.shape
    _grad_close(f"{head} fused={fused} grad_x", xd.grad, g[f"{head}.grad_x"])
    assert all(p.grad is not None for p in m.shapelets.parameters())


# ------------------------------------------------------------------------------------------------------- instance norm
def test_instnorm_bwd_matches_float64_autograd():
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    from oracle import ign_oracle as O
    gen = torch.Generator().manual_seed(2)
    for (B, T, C) in [(3, 100, 6), (2, 1000, 122), (5, 37, 17), (1, 64, 1), (1, 1300, 3)]:
        x = torch.randn(B, T, C, generator=gen) * 3.0 + 50.0          # large offset: the two-pass statistics matter
        gy = torch.randn(B, C, T, generator=gen)
        x64 = x.double().requires_grad_(True)
        O.instance_norm(x64).backward(gy.double())
        xd = x.to(dev).requires_grad_(True)
        xn, xt = ops.instance_norm(xd)
        assert xt is None and xn.requires_grad
        xn.backward(gy.to(dev))
        assert xd.grad.shape == (B, T, C)
        _grad_close(f"instnorm_bwd {B},{T},{C}", xd.grad, x64.grad)


def test_instnorm_bwd_raw_transpose_and_constant_rows():
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 50, 5, generator=gen)
    x[1, :, 3] = 0.75                                                # a constant row: sigma = 0
    gy, gt = torch.randn(2, 5, 50, generator=gen), torch.randn(2, 5, 50, generator=gen)
    xd = x.to(dev).requires_grad_(True)
    xn, xt = ops.instance_norm(xd, want_raw=True)
    (xn * gy.to(dev)).sum().backward(retain_graph=True)
    g_norm = xd.grad.clone()
    assert torch.isfinite(g_norm).all()
    assert float(g_norm[1, :, 3].abs().max()) == 0.0                 # documented: zeros where the reference has NaN
    xd.grad = None
    ((xn * gy.to(dev)).sum() + (xt * gt.to(dev)).sum()).backward()
    assert torch.equal(xd.grad, g_norm + gt.to(dev).permute(0, 2, 1))
    # the plain call is not a node and returns the same bits
    xn0, _ = ops.instance_norm(x.to(dev))
    assert not xn0.requires_grad and torch.equal(xn0, xn.detach())
    with torch.no_grad():
        assert not ops.instance_norm(xd)[0].requires_grad


# ------------------------------------------------------------------------------------------------------- random cases
#       id                  dist gate  B  C  T     Ks         Ls              strides
CASES = [
    ("l1-rbf",              L1,  RBF,  2, 3, 70,   (3,),      (11,),          (1,)),
    ("mse-rbf",             MSE, RBF,  2, 3, 70,   (3,),      (11,),          (1,)),
    ("l1-lts",              L1,  LTS,  2, 3, 70,   (3,),      (11,),          (1,)),
    ("mse-lts",             MSE, LTS,  2, 3, 70,   (3,),      (11,),          (1,)),
    ("l1-rbf-stride3",      L1,  RBF,  2, 3, 100,  (3,),      (17,),          (3,)),
    ("mse-lts-stride3",     MSE, LTS,  2, 3, 100,  (3,),      (17,),          (3,)),
    ("l1-lts-stride3",      L1,  LTS,  2, 2, 101,  (1,),      (16,),          (3,)),      # samples at the end no window covers
    ("l1-rbf-bank",         L1,  RBF,  3, 5, 90,   (2, 3, 5), (7, 20, 33),    (1, 1, 1)),
    ("mse-lts-bank-mixed",  MSE, LTS,  2, 3, 120,  (3, 2),    (9, 40),        (1, 3)),
    ("l1-rbf-T1300",        L1,  RBF,  1, 2, 1300, (2,),      (130,),         (1,)),      # two sample tiles per row
    ("l1-lts-long",         L1,  LTS,  1, 2, 1300, (2,),      (700,),         (1,)),      # two chunks of shapelet positions
    ("mse-rbf-long",        MSE, RBF,  1, 2, 1300, (3,),      (1100,),        (1,)),      # three chunks, K odd
    ("l1-rbf-long-stride3", L1,  RBF,  1, 2, 1300, (2,),      (600,),         (3,)),      # strided, two chunks of offsets
]


def _case_tensors(seed, B, C, T, Ks, Ls):
    gen = torch.Generator().manual_seed(seed)
    xn = torch.randn(B, C, T, generator=gen)
    ws = [torch.randn(K, C, L, generator=gen) for K, L in zip(Ks, Ls)]
    thrs = [torch.rand(1, K, C, generator=gen) for K in Ks]
    r = torch.randn(B, sum(Ks) * C, generator=gen)
    # Seeded normal draws do collide bit for bit once a channel sees ~1e7 (sample, weight) pairs (the default bank at T = 1000 has
    # a few dozen met ties).  The last mantissa bit is therefore cleared in every sample and set in every weight -- a change of
    # half an ulp at most, made to the INPUTS before either side sees them -- and _assert_no_ties then checks the condition.
    xn = (xn.view(torch.int32) & ~1).view(torch.float32)
    ws = [(w.view(torch.int32) | 1).view(torch.float32) for w in ws]
    return xn, ws, thrs, r


@pytest.mark.parametrize("name,dist,gate,B,C,T,Ks,Ls,strides", CASES, ids=[c[0] for c in CASES])
def test_input_grad_matches_the_oracle(name, dist, gate, B, C, T, Ks, Ls, strides):
    dev = _dev()
    xn, ws, thrs, r = _case_tensors(500 + len(name) + T, B, C, T, Ks, Ls)
    _assert_no_ties(xn, ws, strides)
    eps = 0.8
    P0, gx0, gw0, gt0 = _oracle_bank(xn, ws, thrs, eps, dist, gate, strides, r)
    P, gx, gw, gt = _hip_bank(dev, xn, ws, thrs, eps, dist, gate, strides, r)
    parity(f"{name} P", P, P0, tol=1e-4, kind="elem", ref_is="oracle float64")
    parity(f"{name} grad_xn", gx, gx0, tol=1e-4, kind="scale", floor=1e-12, ref_is="oracle float64")
    for i in range(len(ws)):
        parity(f"{name} grad_w{i}", gw[i], gw0[i], tol=1e-4, kind="scale", floor=1e-12, ref_is="oracle float64")


def test_driver_default_bank_input_grad_matches_the_oracle():
    """C=122, T=1000, B=2, four groups of K=5 with L = 100 / 200 / 300 / 500: the bank of the benchmark shape.  The kernels run
    all 122 channels; channels are independent (feature k*C + c reads channel c only), so the float64 oracle is run on 14 of
    them -- first, last, and around the multiples of 32 -- which keeps the test at a couple of seconds instead of twenty."""
    dev = _dev()
    B, C, T, Ks, Ls = 2, 122, 1000, (5, 5, 5, 5), (100, 200, 300, 500)
    xn, ws, thrs, r = _case_tensors(77, B, C, T, Ks, Ls)
    _assert_no_ties(xn, ws)
    P, gx, _, _ = _hip_bank(dev, xn, ws, thrs, 1.0, L1, RBF, (1, 1, 1, 1), r)
    assert gx.shape == (B, C, T)
    ch = torch.tensor([0, 1, 31, 32, 33, 60, 61, 63, 64, 90, 118, 119, 120, 121])
    cols = torch.cat([g * 5 * C + k * C + ch for g in range(4) for k in range(5)])       # g-major, then k, then c: the sub-bank's order
    P0, gx0, _, _ = _oracle_bank(xn[:, ch], [w[:, ch] for w in ws], thrs, 1.0, L1, RBF, (1, 1, 1, 1), r[:, cols])
    parity("default bank P", P.cpu()[:, cols], P0, tol=1e-4, kind="elem", ref_is="oracle float64")
    parity("default bank grad_xn", gx.cpu()[:, ch], gx0, tol=1e-4, kind="scale", floor=1e-12, ref_is="oracle float64")
    # every other channel: finite, and no row left unwritten (each row sums thousands of non-zero terms)
    assert torch.isfinite(gx).all() and float(gx.abs().amax(dim=2).min()) > 0.0


@pytest.mark.parametrize("gate,stride", [(RBF, 1), (LTS, 1), (RBF, 2)])
def test_planted_tie_follows_the_documented_sign_convention(gate, stride):
    """include/ign_abi.h: at x[b,c,s] == w[k,c,j] (bit-equal) the L1 term counts as sign(x - w) = -1 where aten::sgn gives 0, so
    gxn = reference - dl/dd / L at that sample, gw = reference + dl/dd / L at that weight (negatives of each other), and nothing
    else moves.  One tie is planted; dl/dd of its window comes from the oracle's autograd."""
    dev = _dev()
    from oracle import ign_oracle as O
    B, C, T, K, L = 2, 3, 64, 2, 9
    xn, ws, thrs, r = _case_tensors(31 + stride, B, C, T, (K,), (L,))
    b0, c0, k0, j0 = 1, 2, 1, 4
    # the tie goes into the best-matching window of (b0, k0, c0), where the straight-through one-hot makes dl/dd large
    t0 = int(O.window_distance(xn, ws[0], stride, O.MODE_L1, chunk=64)[b0, :, k0, c0].argmin())
    s0 = t0 * stride + j0
    ws[0][k0, c0, j0] = xn[b0, c0, s0]
    w = ws[0]
    Tw = (T - L) // stride + 1
    ties = [(s, j) for s in range(T) for j in range(L) for b in range(B) for k in range(K) for c in range(C)
            if float(xn[b, c, s]) == float(w[k, c, j]) and s >= j and (s - j) % stride == 0 and (s - j) // stride < Tw]
    assert ties == [(s0, j0)]
    x64 = xn.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    d = O.window_distance(x64, w64, stride, O.MODE_L1, chunk=64)
    d.retain_grad()
    P0 = O.lts_softmin_gate(d, thrs[0].double())[0] if gate == LTS else O.rbf_straight_through_max(d, 0.8)[0]
    (P0 * r.double()).sum().backward()
    assert int(d[b0, :, k0, c0].argmin()) == t0                       # still the best window after planting
    term = float(d.grad[b0, t0, k0, c0]) / L                          # dl/dd / L of the tied window
    assert abs(term) > 1e-3 * float(x64.grad.abs().max())             # the convention is visible at the tolerance used
    want_x, want_w = x64.grad.clone(), w64.grad.clone()
    want_x[b0, c0, s0] -= term
    want_w[k0, c0, j0] += term
    _, gx, gw, _ = _hip_bank(dev, xn, ws, thrs, 0.8, L1, gate, (stride,), r)
    parity(f"tie gate={gate} stride={stride} grad_xn", gx, want_x, tol=1e-4, kind="scale", floor=1e-12, ref_is="oracle float64 - dl/dd / L")
    parity(f"tie gate={gate} stride={stride} grad_w", gw[0], want_w, tol=1e-4, kind="scale", floor=1e-12, ref_is="oracle float64 + dl/dd / L")


# --------------------------------------------------------------------------------------------------------- properties
def test_input_grad_is_bitwise_repeatable_and_bank_equals_groups():
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    xn, ws, thrs, r = _case_tensors(9, 3, 5, 1100, (5, 3, 4), (40, 110, 600))
    runs = [_hip_bank(dev, xn, ws, thrs, 0.9, L1, LTS, (1, 1, 1), r)[1] for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    # the bank call = the groups one after another, the first overwriting and the others adding
    x = xn.to(dev).requires_grad_(True)
    wd, td, rd = [w.to(dev) for w in ws], [t.to(dev) for t in thrs], r.to(dev)
    col, acc = 0, None
    for w, t in zip(wd, td):
        n = w.shape[0] * w.shape[1]
        p, _ = ops.shapelet_bank(x, [w], 0.9, L1 | LTS, [1], [t])
        gi, = torch.autograd.grad((p * rd[:, col:col + n]).sum(), x)
        acc = gi if acc is None else acc + gi
        col += n
    assert torch.equal(acc, runs[0])


def test_nine_group_bank_input_grad_equals_the_sum_of_the_groups():
    """More groups than one ign_shapelet_bwd_input_bank call takes (ops.BANK_MAX_GROUPS = 8): the per-group entry point runs nine
    times, the first overwriting and the others adding in place, in group order.  K = 5, L = 5, 8, ..., 29, the fifth group at
    stride 2.  Compared as the multi-group case above compares its bank of three: torch.equal with the group gradients added in
    the same order (every sample is one fp32 add per group on either side)."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    Ls = tuple(range(5, 30, 3))
    strides = tuple(2 if i == 4 else 1 for i in range(len(Ls)))
    assert len(Ls) == 9
    xn, ws, thrs, r = _case_tensors(99, 2, 4, 64, (5,) * len(Ls), Ls)
    _, gx, _, _ = _hip_bank(dev, xn, ws, thrs, 0.9, L1, RBF, strides, r)
    x = xn.to(dev).requires_grad_(True)
    rd = r.to(dev)
    col, acc = 0, None
    for w, stride in zip(ws, strides):
        n = w.shape[0] * w.shape[1]
        p, _ = ops.shapelet_bank(x, [w.to(dev)], 0.9, L1 | RBF, [stride])
        gi, = torch.autograd.grad((p * rd[:, col:col + n]).sum(), x)
        acc = gi if acc is None else acc + gi
        col += n
    assert gx.shape == xn.shape and float(gx.abs().max()) > 0.0
    assert torch.equal(acc, gx)


@pytest.mark.parametrize("cls_name", ["ShapeBottleneckModel", "DistThresholdSBM"])
def test_parameter_grads_do_not_depend_on_x_requires_grad(cls_name):
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from models import Shapelet as S
    torch.manual_seed(4)
    m = getattr(S, cls_name)(make_cfg(enc_in=5, seq_len=80, num_class=3, c_out=3, dec_in=5)).to(dev).train()
    x = torch.randn(6, 80, 5, generator=torch.Generator().manual_seed(5)).to(dev)
    y = (torch.arange(6) % 3).to(dev)
    grads = []
    for need_x in (False, True):
        m.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_(need_x)
        out, info = m(xd)
        (torch.nn.functional.cross_entropy(out, y) + info.loss.mean()).backward()
        assert (xd.grad is not None) == need_x
        grads.append({n: p.grad.clone() for n, p in m.named_parameters()})
    assert set(grads[0]) == set(grads[1]) and all(torch.equal(grads[0][n], grads[1][n]) for n in grads[0])


@pytest.mark.parametrize("dfunc", ["cosine", "pearson"])
def test_cosine_and_pearson_refuse_an_input_gradient_at_forward_time(dfunc):
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    from ign_hip._lib import IgnError
    from models.Shapelet import ShapeBottleneckModel
    m = ShapeBottleneckModel(make_cfg(enc_in=4, seq_len=60, distance_func=dfunc)).to(dev)
    x = torch.randn(2, 60, 4, device=dev)
    m(x)                                                             # data input: unchanged
    with pytest.raises(IgnError, match="cosine / pearson"):
        m(x.clone().requires_grad_(True))
    xn = torch.randn(2, 4, 60, device=dev, requires_grad=True)
    w = torch.randn(3, 4, 9, device=dev, requires_grad=True)
    with pytest.raises(IgnError, match="cosine / pearson"):
        ops.shapelet_bank(xn, [w], 1.0, COS if dfunc == "cosine" else PEARSON)


# ----------------------------------------------------------------------------------------------------------- saliency
def _oracle_saliency(m, x, lts, idx):
    from oracle import ign_oracle as O
    ref = O.OracleSBM(m.configs, num_shapelet=m.num_shapelet, shapelet_len=(0.1, 0.2, 0.3, 0.5), lts=lts, chunk=64)
    ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    ref = ref.double().eval()
    x64 = x.detach().cpu().double().requires_grad_(True)
    out, _ = ref(x64)
    out.gather(1, idx.cpu()[:, None]).sum().backward()
    return out.detach(), x64.grad


@pytest.mark.parametrize("kind", ["SBM", "LTS", "InterpGN"])
def test_input_saliency(kind):
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import _lib
    from models.InterpGN import InterpGN
    from models.Shapelet import DistThresholdSBM, ShapeBottleneckModel
    from utils.saliency import input_saliency
    torch.manual_seed(6)
    cfg = make_cfg(enc_in=5, seq_len=80, num_class=4, c_out=4, dec_in=5)
    m = {"SBM": ShapeBottleneckModel, "LTS": DistThresholdSBM, "InterpGN": InterpGN}[kind](cfg).to(dev).train()
    expert = m.sbm if kind == "InterpGN" else m
    B = 4
    x = torch.randn(B, 80, 5, generator=torch.Generator().manual_seed(7)).to(dev)
    from oracle import ign_oracle as O
    _assert_no_ties(O.instance_norm(x.cpu()), [s.weights for s in expert.shapelets])      # the bank meets the NORMALISED series
    required = [p.requires_grad for p in m.parameters()]
    expert.dropout.eval()                                            # a mixed train / eval set-up must come back as it was
    modes = [mod.training for mod in m.modules()]

    _lib.timing_enable(True)
    sal = input_saliency(m, x)                                       # predicted class
    _, n_w = _lib.timing_read("shp_bwd")
    _, n_r = _lib.timing_read("reduce_parts")
    _, n_x = _lib.timing_read("shp_bwd_x")
    _, n_n = _lib.timing_read("instnorm_bwd")
    _lib.timing_enable(False)
    assert sal.shape == x.shape and sal.device == x.device and torch.isfinite(sal).all()
    assert n_w == 0 and n_r == 0, "saliency must not run the weight-backward launches"
    assert n_x == len(expert.shapelets) and n_n == 1
    assert all(p.grad is None for p in m.parameters())
    assert [p.requires_grad for p in m.parameters()] == required and m.training and not x.requires_grad
    assert [mod.training for mod in m.modules()] == modes and not expert.dropout.training

    with torch.no_grad():
        logits = expert.eval()(x)[0]
        expert.train()
    pred = logits.argmax(dim=1)
    out0, g0 = _oracle_saliency(expert, x, kind == "LTS", pred)
    parity(f"{kind} logits", logits, out0, tol=1e-4, kind="elem", ref_is="oracle float64")
    parity(f"{kind} saliency(pred)", sal, g0, tol=1e-4, kind="scale", floor=1e-12, ref_is="oracle float64")
    assert torch.equal(input_saliency(m, x, pred), sal)              # a (B,) tensor
    tgt = torch.full((B,), 2, dtype=torch.long)
    _, g2 = _oracle_saliency(expert, x, kind == "LTS", tgt)
    parity(f"{kind} saliency(2)", input_saliency(m, x, 2), g2, tol=1e-4, kind="scale", floor=1e-12, ref_is="oracle float64")
    with pytest.raises(ValueError):
        input_saliency(m, x, 4)
    if kind == "InterpGN":
        # the deep expert has no input gradient and says so
        xd = x.clone().requires_grad_(True)
        with pytest.raises(_lib.IgnError, match="input series"):
            m(xd)[0].sum().backward()


def test_experiment_saliency_runs_the_helper_over_a_loader():
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from argparse import Namespace
    from exp.experiment_classification import Experiment
    from models.Shapelet import ShapeBottleneckModel
    from utils.saliency import input_saliency
    torch.manual_seed(8)
    cfg = make_cfg(enc_in=3, seq_len=40, num_class=2, c_out=2, dec_in=3)
    exp = Experiment.__new__(Experiment)
    exp.model, exp.device, exp.args = ShapeBottleneckModel(cfg).to(dev), dev, Namespace(seq_len=40, enc_in=3)
    batches = [(torch.randn(n, 40, 3), torch.zeros(n), torch.ones(n, 40)) for n in (3, 2)]
    exp.test_loader = batches
    sal = exp.saliency(target=1)
    assert sal.shape == (5, 40, 3) and sal.device.type == "cpu"
    assert torch.equal(sal[3:], input_saliency(exp.model, batches[1][0].to(dev), 1).cpu())
    assert exp.saliency(loader=batches[:1]).shape == (3, 40, 3)
