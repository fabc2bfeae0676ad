"""GPU parity of the opt-in exact-tie L1 backward passes (IGN_TIE_EXACT, mode bit 0x20; include/ign_abi.h): with the bit an element
with x[b,c,s] == w[k,c,j] (bit-equal floats) contributes 0 to gw and gxn, as the reference's aten::sgn does, so both equal the
reference's unmodified gradient -- the fixtures tests/golden/shapelet_tie_{l1,lts}.npz directly, and float64 autograd of the CPU
oracle (torch.sign, sign(0) = 0) on seeded inputs dense with ties, for every kernel body of the two passes.  Every comparison goes
through conftest.parity at 1e-4; each case also runs WITHOUT the bit and must then miss the same reference, so the inputs are
shown to exercise the switch.  The default convention itself stays pinned by test_gpu_shapelet.py / test_gpu_input_grad.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, make_cfg, parity

pytestmark = pytest.mark.gpu

L1, MSE = 0, 1
RBF, LTS = 0x00, 0x10
TIE = 0x20
TOL = 1e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _t(a, dev=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev) if dev is not None else t


def _grad(label, got, ref, ref_is="oracle float64"):
    return parity(label, got, ref, tol=TOL, kind="scale", floor=1e-12, ref_is=ref_is)


def _misses(got, ref):
    """max |got - ref| relative to the reference's scale -- the measure _grad judges -- is beyond the tolerance"""
    g, r = got.detach().double().cpu(), torch.as_tensor(ref).double()
    return float((g - r).abs().max()) > TOL * float(r.abs().max())


def _hip(dev, xn, w, thr, eps, mode, stride, r, x_grad=True):
    """sum(P * r) through ops.shapelet_bank in `mode`: -> (P, Dmin, grad_xn, grad_w, grad_thr)"""
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    x = xn.to(dev).requires_grad_(x_grad)
    wd = w.to(dev).requires_grad_(True)
    td = thr.to(dev).requires_grad_(True) if mode & LTS else None
    P, D = ops.shapelet_bank(x, [wd], eps, mode, [stride], [td] if td is not None else None)
    (P * r.to(dev)).sum().backward()
    return P.detach(), D.detach(), x.grad, wd.grad, (td.grad if td is not None else None)


def _oracle(xn, w, thr, eps, gate, stride, r, mse=False):
    """the same expression through the oracle in float64 (torch.sign in its backward: sign(0) = 0): -> (P, d, grad_xn, grad_w, grad_thr)"""
    from oracle import ign_oracle as O
    x = xn.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    t64 = thr.double().requires_grad_(True) if gate == LTS else None
    d = O.window_distance(x, w64, stride, O.MODE_MSE if mse else O.MODE_L1, chunk=64)
    P = O.lts_softmin_gate(d, t64)[0] if gate == LTS else O.rbf_straight_through_max(d, eps)[0]
    grads = torch.autograd.grad((P * r.double()).sum(), [x, w64] + ([t64] if gate == LTS else []))
    return P.detach(), d.detach(), grads[0], grads[1], (grads[2] if gate == LTS else None)


# ------------------------------------------------------------------------------------------------ A / B: the reference fixtures
@pytest.mark.parametrize("name", ["l1", "lts"])
def test_fixture_weight_gradient_is_the_references_own(name):
    """A.  B 3, C 4, T 60, K 3, L 9: one shapelet a copy of a window plus three single ties, gradient recorded from the
    reference.  With the bit w.grad is g["grad_w"] itself -- no tie term subtracted; without it the same call misses it."""
    dev = _dev()
    g = golden(f"shapelet_tie_{name}")
    gate = LTS if name == "lts" else RBF
    xn, w, r = _t(g["xn"]), _t(g["w"]), _t(g["r"])
    thr = _t(g["thr"]) if gate == LTS else None
    eps = float(g["eps"])
    P, D, _, gw, gt = _hip(dev, xn, w, thr, eps, L1 | gate | TIE, 1, r, x_grad=False)
    parity(f"tie-exact {name} p", P, g["p"], tol=TOL, kind="elem")
    parity(f"tie-exact {name} dmin", D, g["dmin"], tol=TOL, kind="elem")
    _grad(f"tie-exact {name} grad_w", gw, g["grad_w"], ref_is="reference fp32")
    if gate == LTS:
        _grad(f"tie-exact {name} grad_thr", gt, g["grad_thr"], ref_is="reference fp32")
    P0, D0, _, gw0, _ = _hip(dev, xn, w, thr, eps, L1 | gate, 1, r, x_grad=False)
    assert torch.equal(P0, P) and torch.equal(D0, D)                 # the forward ignores the bit
    assert _misses(gw0, g["grad_w"]), "the fixture does not exercise the switch"


@pytest.mark.parametrize("name", ["l1", "lts"])
def test_fixture_input_gradient_matches_oracle_autograd(name):
    """B.  xn.grad of the same expression with the bit: float64 autograd of the oracle; w.grad of the same backward: the fixture."""
    dev = _dev()
    g = golden(f"shapelet_tie_{name}")
    gate = LTS if name == "lts" else RBF
    xn, w, r = _t(g["xn"]), _t(g["w"]), _t(g["r"])
    thr = _t(g["thr"]) if gate == LTS else None
    eps = float(g["eps"])
    _, _, gx0, gw0, _ = _oracle(xn, w, thr, eps, gate, 1, r)
    _, _, gx, gw, _ = _hip(dev, xn, w, thr, eps, L1 | gate | TIE, 1, r)
    _grad(f"tie-exact {name} grad_xn", gx, gx0)
    _grad(f"tie-exact {name} grad_w (with the input pass)", gw, g["grad_w"], ref_is="reference fp32")
    parity(f"oracle {name} grad_w vs fixture", gw0, g["grad_w"], tol=TOL, kind="scale", floor=1e-12, ref_is="reference fp32")


# ------------------------------------------------------------------------------------------------ C: dense ties, all kernel bodies
def _plan(K, L, Tw):
    """plan_bwd of csrc/ign_abi.hip for stride 1, restated: -> (JJ, chunks of the window axis).  JJ maximises
    eff = kb*L / (threads*JJ), x 1.10 for JJ = 8 (tried first); kb then maximises lane use; ~5 KB of LDS per wave bound tc."""
    best, best_eff = 0, -1.0
    for JJ in (8, 4):
        cpk = -(-L // JJ)
        if cpk > 512:
            continue
        kb = max(1, min(K, 512 // cpk))
        threads = -(-kb * cpk // 64) * 64
        eff = kb * L / (threads * JJ) * (1.10 if JJ == 8 else 1.0)
        if eff > best_eff:
            best, best_eff = JJ, eff
    JJ = best
    cpk = -(-L // JJ)
    kb, best_u = 1, -1.0
    for k in range(1, K + 1):
        if k * cpk > 512:
            break
        u = K * cpk / (-(-K // k) * (-(-k * cpk // 64) * 64))
        if u > best_u + 1e-9:
            kb, best_u = k, u
    threads = -(-kb * cpk // 64) * 64
    budget = max(8 * 1024, threads // 64 * 5 * 1024)
    tc_max = (budget // 4 - (cpk * JJ + 16 * kb + 8)) // (1 + kb)
    tc_max = max(2 * JJ, tc_max // (2 * JJ) * (2 * JJ))
    return JJ, -(-Tw // tc_max)


#        id            K  L    T     stride gate  seed  weight-pass body            JJ    window chunks  input-pass position chunks
DENSE = [
    ("jj4",            3, 9,   64,   1,     RBF,  0,    "stride 1",                 4,    1,             1),
    ("jj8",            8, 64,  200,  1,     LTS,  0,    "stride 1",                 8,    1,             1),
    ("strided",        2, 9,   64,   3,     RBF,  175,  "strided",                  4,    None,          1),
    ("long",           2, 600, 1100, 1,     LTS,  0,    "stride 1",                 4,    1,             2),      # > 512 positions: two walks
    ("jj8-two-chunks", 8, 64,  300,  1,     LTS,  0,    "stride 1",                 8,    2,             1),      # Tw = 237 > tc = 192
]
DENSE_B, DENSE_C = 3, 2
# Under the planner the "long" shape stages its 501 windows in ONE chunk (tc_max = 1920 for its 5-wave block), so the fifth shape is
# there for the second window chunk: a one-wave block (8 KB of LDS) takes 192 windows at a time.
# The seeds were chosen on the CPU from the oracle alone, for the two conditions the test asserts on its inputs (the strided shape
# has only ~2000 (sample, weight) pairs: seed 175 is the first with a count well above 50).


def _dense_inputs(seed, K, L, T):
    """seeded normal draws; a random third of the samples and of the weights snapped to a grid of step 0.5 (many exact ties),
    the rest continuous (window distances do not tie)"""
    gen = torch.Generator().manual_seed(1000 + seed)
    xn = torch.randn(DENSE_B, DENSE_C, T, generator=gen)
    w = torch.randn(K, DENSE_C, L, generator=gen)
    mx = torch.rand(xn.shape, generator=gen) < 1.0 / 3.0
    mw = torch.rand(w.shape, generator=gen) < 1.0 / 3.0
    xn = torch.where(mx, torch.round(xn * 2) / 2, xn)
    w = torch.where(mw, torch.round(w * 2) / 2, w)
    thr = torch.rand(1, K, DENSE_C, generator=gen)
    r = torch.randn(DENSE_B, K * DENSE_C, generator=gen)
    return xn, w, thr, r


def _count_ties(xn, w, stride):
    win = xn.unfold(2, w.shape[2], stride)                             # (B, C, Tw, L): sample t*stride + j meets position j
    return int((win.permute(0, 2, 1, 3).unsqueeze(2) == w.unsqueeze(0).unsqueeze(0)).sum())


_DENSE_CACHE = {}


def _dense_case(name):
    """inputs, the float64 oracle's results and the conditions on the inputs, computed once per case and left unchanged"""
    if name not in _DENSE_CACHE:
        _, K, L, T, stride, gate, seed = next(c for c in DENSE if c[0] == name)[:7]
        xn, w, thr, r = _dense_inputs(seed, K, L, T)
        P0, d, gx0, gw0, gt0 = _oracle(xn, w, thr, 0.8, gate, stride, r)
        two = torch.sort(d, dim=1).values[:, :2]                       # both gates pick the window of smallest distance
        gap = float((two[:, 1] - two[:, 0]).min())
        _DENSE_CACHE[name] = dict(xn=xn, w=w, thr=thr, r=r, P0=P0, gx0=gx0, gw0=gw0, gt0=gt0, ties=_count_ties(xn, w, stride), gap=gap)
    return _DENSE_CACHE[name]


@pytest.mark.parametrize("name,K,L,T,stride,gate,seed,body,JJ,wchunks,pchunks", DENSE, ids=[c[0] for c in DENSE])
def test_dense_ties_match_oracle_autograd(name, K, L, T, stride, gate, seed, body, JJ, wchunks, pchunks):
    dev = _dev()
    Tw = (T - L) // stride + 1
    # which kernel body the shape reaches (a planner change must not silently drop coverage)
    if stride == 1:
        assert _plan(K, L, Tw) == (JJ, wchunks), _plan(K, L, Tw)
    else:
        assert body == "strided" and JJ == 4                          # plan_bwd_strided: always JJ = 4
    M = -(-L // stride)
    assert -(-M // min(M, max(1, 512 // stride))) == pchunks          # ign_bwdx_plan: mc = min(M, max(1, 512 / stride)) offsets per chunk
    c = _dense_case(name)
    # the conditions on the inputs
    assert c["ties"] >= 50, c["ties"]
    assert c["gap"] > 1e-6, f"two best windows of a row {c['gap']} apart"      # every (b, k, c) row is compared: share left out = 0
    P, _, gx, gw, gt = _hip(dev, c["xn"], c["w"], c["thr"], 0.8, L1 | gate | TIE, stride, c["r"])
    parity(f"{name} P", P, c["P0"], tol=TOL, kind="elem", ref_is="oracle float64")
    _grad(f"{name} grad_w", gw, c["gw0"])
    _grad(f"{name} grad_xn", gx, c["gx0"])
    if gate == LTS:
        _grad(f"{name} grad_thr", gt, c["gt0"])
    _, _, gx_d, gw_d, _ = _hip(dev, c["xn"], c["w"], c["thr"], 0.8, L1 | gate, stride, c["r"])
    assert _misses(gw_d, c["gw0"]), "without the bit the weight gradient should miss the oracle on these inputs"


# ------------------------------------------------------------------------------------------------ D: through the model
@pytest.mark.parametrize("cls_name", ["ShapeBottleneckModel", "DistThresholdSBM"])
def test_model_with_copied_windows_matches_the_oracle(cls_name):
    """D.  The data-driven initialisation: the first shapelet of every group is a copy of a window of the instance-normalised
    batch, so it ties with that window at every position.  Each side copies from ITS OWN normalised batch (the kernel's fp32
    instance norm here, the oracle's float64 one there): a copy is a tie by construction on either side, and the two copies
    differ by the fp32 rounding of the normalisation, far below the tolerance.  One backward of cross_entropy + info.loss through
    the fused node (linear head), every parameter gradient and the saliency against the oracle's model in float64."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    from models import Shapelet as S
    from oracle import ign_oracle as O
    from utils.saliency import input_saliency
    lts = cls_name == "DistThresholdSBM"
    torch.manual_seed(11)
    cfg = make_cfg(enc_in=3, seq_len=60, num_class=3, c_out=3, dec_in=3)
    m = getattr(S, cls_name)(cfg, num_shapelet=[2] * 4).to(dev).train()
    ref = O.OracleSBM(cfg, num_shapelet=[2] * 4, lts=lts, chunk=64)
    ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    ref = ref.double().train()
    Bm, b0, t0 = 4, 1, 7
    x = torch.randn(Bm, 60, 3, generator=torch.Generator().manual_seed(12))
    y = torch.arange(Bm) % 3
    xn_hip, _ = ops.instance_norm(x.to(dev))
    xn_ref = O.instance_norm(x.double())
    with torch.no_grad():
        for s, so in zip(m.shapelets, ref.shapelets):
            s.weights[0] = xn_hip[b0, :, t0:t0 + s.length]
            so.weights[0] = xn_ref[b0, :, t0:t0 + s.length]
            assert torch.equal(s.weights[0], xn_hip[b0, :, t0:t0 + s.length])
    assert m.set_tie_exact(True) is m and all(s.mode() & TIE for s in m.shapelets)

    out0, info0 = ref(x.double())
    (F.cross_entropy(out0, y) + info0.loss.mean()).backward()
    want = {n: p.grad for n, p in ref.named_parameters()}

    def grads():
        m.zero_grad(set_to_none=True)
        out, info = m(x.to(dev))
        (F.cross_entropy(out, y.to(dev)) + info.loss.mean()).backward()
        return out.detach(), {n: p.grad.clone() for n, p in m.named_parameters()}

    out, got = grads()
    parity(f"{cls_name} logits", out, out0.detach(), tol=TOL, kind="elem", ref_is="oracle float64")
    assert set(got) == set(want)
    for n in sorted(want):
        _grad(f"{cls_name} {n}", got[n], want[n])

    with torch.no_grad():
        pred = m.eval()(x.to(dev))[0].argmax(dim=1).cpu()
        m.train()
    x64 = x.double().requires_grad_(True)
    ref.eval()(x64)[0].gather(1, pred[:, None]).sum().backward()
    _grad(f"{cls_name} saliency", input_saliency(m, x.to(dev)), x64.grad)

    if lts:       # the perfect-match window carries gradient under the LTS gate: the default convention misses the oracle here
        m.set_tie_exact(False)
        _, plain = grads()
        assert any(_misses(plain[n], want[n]) for n in want if n.endswith(".weights"))


# ------------------------------------------------------------------------------------------------ E: properties with the bit set
def test_exact_tie_passes_are_bitwise_repeatable():
    dev = _dev()
    c = _dense_case("jj8")
    runs = [_hip(dev, c["xn"], c["w"], c["thr"], 0.8, L1 | LTS | TIE, 1, c["r"]) for _ in range(2)]
    assert torch.equal(runs[0][3], runs[1][3]) and torch.equal(runs[0][2], runs[1][2])


@pytest.mark.parametrize("K,L,T,stride,gate", [(3, 9, 64, 1, RBF), (8, 64, 200, 1, LTS), (2, 9, 64, 3, RBF)])
def test_tie_free_inputs_agree_with_the_default(K, L, T, stride, gate):
    """no sample is bit-equal to a weight (last mantissa bit cleared in the samples, set in the weights, as
    tests/test_gpu_input_grad.py does): the two conventions compute the same sums, up to rounding"""
    dev = _dev()
    gen = torch.Generator().manual_seed(77)
    xn = (torch.randn(DENSE_B, DENSE_C, T, generator=gen).view(torch.int32) & ~1).view(torch.float32)
    w = (torch.randn(K, DENSE_C, L, generator=gen).view(torch.int32) | 1).view(torch.float32)
    thr = torch.rand(1, K, DENSE_C, generator=gen)
    r = torch.randn(DENSE_B, K * DENSE_C, generator=gen)
    assert _count_ties(xn, w, stride) == 0
    P, D, gx, gw, gt = _hip(dev, xn, w, thr, 0.8, L1 | gate | TIE, stride, r)
    P0, D0, gx0, gw0, gt0 = _hip(dev, xn, w, thr, 0.8, L1 | gate, stride, r)
    assert torch.equal(P, P0) and torch.equal(D, D0)
    _grad(f"tie-free {K},{L},{T},{stride} grad_w", gw, gw0, ref_is="the default kernels")
    _grad(f"tie-free {K},{L},{T},{stride} grad_xn", gx, gx0, ref_is="the default kernels")
    if gate == LTS:
        assert torch.equal(gt, gt0)


@pytest.mark.parametrize("gate,stride", [(RBF, 1), (LTS, 3)])
def test_mse_ignores_the_bit_bitwise(gate, stride):
    dev = _dev()
    xn, w, thr, r = _dense_inputs(5, 3, 9, 64)
    a = _hip(dev, xn, w, thr, 0.8, MSE | gate | TIE, stride, r)
    b = _hip(dev, xn, w, thr, 0.8, MSE | gate, stride, r)
    assert all(u is None and v is None or torch.equal(u, v) for u, v in zip(a, b))
    assert float(a[3].abs().max()) > 0.0 and float(a[2].abs().max()) > 0.0
