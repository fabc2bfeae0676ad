"""GPU parity of --mask_padding: ign_instnorm_fwd_len and ign_shapelet_regate (csrc/ign_shapelet_mask.hip) behind the unchanged
shapelet forward / backward kernels, their ops (instance_norm_len, shapelet_bank(lengths=)) and the masked SBM / LTS / InterpGN
models.  The specification is "sample b as if it had been given alone, truncated to its length n_b": the expected values are the
CPU oracle (oracle/ign_oracle.py) in float64 applied sample by sample to x[b, :n_b], gradients the float64 autograd of sum(r * P)
summed over the samples.  Comparisons go through conftest.parity at 1e-4: kind="elem" for xn, P and Dmin, kind="scale",
floor=1e-12 for gradients (the rule of tests/test_gpu_input_grad.py).  The gradient tests are also what verifies that the saved
distance 1e18 of an invalid window contributes exactly nothing in the existing backward kernels.

Inputs: torch.Generator().manual_seed(s); x = randn(B, T, C) first, then w_g = randn(K_g, C, L_g) per group, then (left to this
file) thr_g = rand(1, K_g, C) per group and r = randn(B, F), all float64, then cast; x is zeroed from n_b on, as the loader pads.
  A (seed 0)  B=6 C=3 T=96, K=(3,2) L=(8,40) stride 1, lengths [96,40,39,8,7,57]: full length, exactly one window, one sample
              short of a window, one group empty while the other is not, no window at all
  B (seed 1)  B=4 C=2 T=120, K=3 L=16 stride 3, lengths [120,61,16,18]: stride, lengths that do not fall on the stride
  C (seed 2)  B=3 C=2 T=700, K=2 L=20, lengths [700,333,20]: Tw = 681, several trips of the kernel's row loop
"""
import functools

import numpy as np
import pytest
import torch

from conftest import golden, make_cfg, parity, sd_from

pytestmark = pytest.mark.gpu

L1, MSE, COS, PEARSON = 0, 1, 2, 3
RBF, LTS = 0x00, 0x10
EPS = 1.0
SHAPES = {
    "A": dict(seed=0, B=6, C=3, T=96, K=(3, 2), L=(8, 40), stride=(1, 1), lengths=(96, 40, 39, 8, 7, 57)),
    "B": dict(seed=1, B=4, C=2, T=120, K=(3,), L=(16,), stride=(3,), lengths=(120, 61, 16, 18)),
    "C": dict(seed=2, B=3, C=2, T=700, K=(2,), L=(20,), stride=(1,), lengths=(700, 333, 20)),
}
CASES = [(s, L1, g) for s in "ABC" for g in (RBF, LTS)] + [("A", d, RBF) for d in (MSE, COS, PEARSON)]
# Smallest float64 gap between best and runner-up window (in p for RBF, in d for LTS) at which t* is compared on EVERY feature.
# The three L1 recipes were checked on the CPU: >= 6.99e-4 in p and >= 9.11e-4 in d, hence 1e-4.  Shape A with MSE / cosine has
# 2.76e-3 / 1.96e-3, with pearson 9.73e-5 -- below 1e-4 by the draw, not by the code -- so the other distances take a bound worked
# out from the fp32 arithmetic instead: a distance is a mean or a normalised dot product of L <= 40 terms, each rounded to 2^-24
# relative (|delta d| <= ~40 * 6e-8 * sum|terms|/L ~ 1e-5 for O(1) operands); |dp/dd| = 2 eps^2 d p <= 0.86, plus __expf's ~2e-6
# relative error: |delta p| < 1.5e-5 per window, 3e-5 between two of them.  5e-5 leaves room above that.
GAP_MIN = {L1: 1e-4, MSE: 5e-5, COS: 5e-5, PEARSON: 5e-5}
IDS = [f"{s}-{('l1', 'mse', 'cos', 'pearson')[d]}-{'lts' if g else 'rbf'}" for s, d, g in CASES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ops():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    return ops


def _grad_close(label, got, ref):
    return parity(label, got, ref, tol=1e-4, kind="scale", floor=1e-12)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """-> dict(x (B,T,C) zero-padded, ws, thrs, r, lengths), float64 on the CPU; read-only, shared by every test of the shape"""
    s = SHAPES[shape]
    g = torch.Generator().manual_seed(s["seed"])
    x = torch.randn(s["B"], s["T"], s["C"], generator=g, dtype=torch.float64)
    ws = [torch.randn(K, s["C"], L, generator=g, dtype=torch.float64) for K, L in zip(s["K"], s["L"])]
    thrs = [torch.rand(1, K, s["C"], generator=g, dtype=torch.float64) for K in s["K"]]
    r = torch.randn(s["B"], sum(s["K"]) * s["C"], generator=g, dtype=torch.float64)
    for b, n in enumerate(s["lengths"]):
        x[b, n:] = 0.0
    return dict(x=x, ws=ws, thrs=thrs, r=r, lengths=list(s["lengths"]), strides=list(s["stride"]))


def _oracle_xn(x, lengths):
    """per-sample instance norm of x[b, :n_b] -> (B,C,T) float64, zeros from n_b on (and everywhere for n_b < 2)"""
    from oracle import ign_oracle as O
    B, T, C = x.shape
    xn = torch.zeros(B, C, T, dtype=torch.float64)
    for b, n in enumerate(lengths):
        if n >= 2:
            xn[b, :, :n] = O.instance_norm(x[b:b + 1, :n].double())[0]
    return xn


def _oracle_sample(xb, ws, thrs, strides, dist, gate):
    """One truncated sample xb (1,n,C) float64 through the oracle: -> (P (F), Dmin (F), t* (F) int, gap (F)) with P = 0,
    Dmin = NO_WINDOW, t* = -1, gap = inf on the features of a group the sample is too short for; P carries the autograd graph.
    gap: best minus runner-up of p (RBF) / runner-up minus best of d (LTS), inf for a single window."""
    from oracle import ign_oracle as O
    NO_WINDOW = _ops().NO_WINDOW
    n = xb.shape[1]
    xn = O.instance_norm(xb) if n >= 2 else None
    Ps, Ds, ts, gaps = [], [], [], []
    for g, w in enumerate(ws):
        K, C, L = w.shape
        if n < L or xn is None:
            Ps.append(torch.zeros(K * C, dtype=torch.float64))
            Ds.append(torch.full((K * C,), NO_WINDOW, dtype=torch.float64))
            ts.append(torch.full((K * C,), -1, dtype=torch.long))
            gaps.append(torch.full((K * C,), float("inf"), dtype=torch.float64))
            continue
        d = O.window_distance(xn, w, strides[g], dist, chunk=64)                    # (1,Tw,K,C)
        P, Dmin = O.lts_softmin_gate(d, thrs[g]) if gate == LTS else O.rbf_straight_through_max(d, EPS)
        score = (-d if gate == LTS else torch.exp(-torch.pow(EPS * d, 2))).detach()[0]      # (Tw,K,C): the arg-max is t*
        ts.append(score.argmax(dim=0).flatten())
        if score.shape[0] > 1:
            top = score.topk(2, dim=0).values
            gaps.append((top[0] - top[1]).flatten())
        else:
            gaps.append(torch.full((K * C,), float("inf"), dtype=torch.float64))
        Ps.append(P[0])
        Ds.append(Dmin[0].detach())
    return torch.cat(Ps), torch.cat(Ds), torch.cat(ts), torch.cat(gaps)


@functools.lru_cache(maxsize=None)
def _oracle(shape, dist, gate):
    """The per-sample float64 reference of one case, computed once: P, Dmin, t*, gap (B,F) and the gradients of sum(r * P)."""
    inp = _inputs(shape)
    ws = [w.clone().requires_grad_(True) for w in inp["ws"]]
    thrs = [t.clone().requires_grad_(True) for t in inp["thrs"]]
    rows = [_oracle_sample(inp["x"][b:b + 1, :n], ws, thrs, inp["strides"], dist, gate) for b, n in enumerate(inp["lengths"])]
    P, D, t, gap = (torch.stack(f) for f in zip(*rows))
    wanted = ws + (thrs if gate == LTS else [])
    grads = torch.autograd.grad((P * inp["r"]).sum(), wanted)
    G = len(ws)
    return dict(P=P.detach(), D=D, t=t, gap=gap, gw=list(grads[:G]), gt=list(grads[G:]))


def _hip(dev, shape, dist, gate, x=None):
    """The same case on the GPU (fp32): -> dict(xn, P, D, t, gw, gt).  `x`: another batch in place of the shape's (same lengths)."""
    ops = _ops()
    inp = _inputs(shape)
    xd = (inp["x"] if x is None else x).float().to(dev)
    lengths = torch.tensor(inp["lengths"], dtype=torch.int32, device=dev)
    xn = ops.instance_norm_len(xd, lengths)
    wd = [w.float().to(dev).requires_grad_(True) for w in inp["ws"]]
    td = [t.float().to(dev).requires_grad_(True) for t in inp["thrs"]] if gate == LTS else None
    P, D, t = ops.shapelet_bank(xn, wd, EPS, dist | gate, inp["strides"], td, return_tstar=True, lengths=lengths)
    (P * inp["r"].float().to(dev)).sum().backward()
    return dict(xn=xn, P=P.detach(), D=D, t=t, gw=[w.grad for w in wd], gt=[t_.grad for t_ in (td or [])])


# ---------------------------------------------------------------------------------------------------------------- instance norm
@pytest.mark.parametrize("shape", list(SHAPES))
def test_instance_norm_len_matches_the_truncated_samples(shape):
    dev = _dev()
    ops = _ops()
    inp = _inputs(shape)
    lengths = torch.tensor(inp["lengths"], dtype=torch.int32, device=dev)
    xn = ops.instance_norm_len(inp["x"].float().to(dev), lengths)
    parity(f"{shape} xn", xn, _oracle_xn(inp["x"], inp["lengths"]), tol=1e-4, kind="elem")
    for b, n in enumerate(inp["lengths"]):
        assert not xn[b, :, n:].any(), f"sample {b}: padding not exactly zero"


def test_instance_norm_len_short_rows_and_garbage_padding():
    """n_b < 2: the whole row is 0; n_b = 2 is normalised; what the padding holds is never read"""
    dev = _dev()
    ops = _ops()
    x = _inputs("A")["x"].clone()
    x[:, 50:] = 1e6                                     # garbage where the lengths below say "padding"
    lens = [1, 0, 2, 50, 3, 17]
    xn = ops.instance_norm_len(x.float().to(dev), torch.tensor(lens, dtype=torch.int32, device=dev))
    assert not xn[0].any() and not xn[1].any()
    parity("short rows xn", xn, _oracle_xn(x, lens), tol=1e-4, kind="elem")
    for b, n in enumerate(lens):
        assert not xn[b, :, n:].any()


# ---------------------------------------------------------------------------------------------------------------- the bank
@pytest.mark.parametrize("shape,dist,gate", CASES, ids=IDS)
def test_bank_matches_the_truncated_samples(shape, dist, gate):
    dev = _dev()
    NO_WINDOW = _ops().NO_WINDOW
    ref, got = _oracle(shape, dist, gate), _hip(dev, shape, dist, gate)
    empty = ref["t"] < 0
    assert bool(empty.any()) == (shape == "A")          # shape A is the one with features that have no window
    P, D, t = got["P"].cpu(), got["D"].cpu(), got["t"].cpu().long()
    # no window: exact values
    assert (P[empty] == 0).all() and (D[empty] == np.float32(NO_WINDOW)).all() and (t[empty] == -1).all()
    parity(f"{shape} P", P, ref["P"], tol=1e-4, kind="elem")
    parity(f"{shape} Dmin", D[~empty], ref["D"][~empty], tol=1e-4, kind="elem")
    # match locations on EVERY non-empty feature: the float64 gap between best and runner-up is far above fp32 resolution
    gap = ref["gap"][~empty]
    print(f"{shape} smallest best/runner-up gap {float(gap.min()):.3e}")
    assert float(gap.min()) > GAP_MIN[dist], "the recipe no longer separates best and runner-up: t* cannot be compared"
    assert torch.equal(t[~empty], ref["t"][~empty])
    for g, (a, b) in enumerate(zip(got["gw"], ref["gw"])):
        _grad_close(f"{shape} grad_w[{g}]", a, b)
    assert len(got["gt"]) == len(ref["gt"])
    for g, (a, b) in enumerate(zip(got["gt"], ref["gt"])):
        _grad_close(f"{shape} grad_thr[{g}]", a, b)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("gate", [RBF, LTS], ids=["rbf", "lts"])
def test_a_full_length_sample_gives_the_unmasked_result(shape, gate):
    """sample 0 of every shape has n_b = T: the masked path must agree with the existing, unmasked one on it"""
    dev = _dev()
    ops = _ops()
    inp = _inputs(shape)
    assert inp["lengths"][0] == SHAPES[shape]["T"]
    got = _hip(dev, shape, L1, gate)
    xn, _ = ops.instance_norm(inp["x"][:1].float().to(dev))
    wd = [w.float().to(dev) for w in inp["ws"]]
    td = [t.float().to(dev) for t in inp["thrs"]] if gate == LTS else None
    P, D, t = ops.shapelet_bank(xn, wd, EPS, L1 | gate, inp["strides"], td, return_tstar=True)
    parity(f"{shape} xn[0]", got["xn"][:1], xn, tol=1e-4, kind="elem", ref_is="unmasked HIP path")
    parity(f"{shape} P[0]", got["P"][:1], P, tol=1e-4, kind="elem", ref_is="unmasked HIP path")
    parity(f"{shape} Dmin[0]", got["D"][:1], D, tol=1e-4, kind="elem", ref_is="unmasked HIP path")
    assert torch.equal(got["t"][:1], t)


@pytest.mark.parametrize("shape,dist,gate", [("A", L1, RBF), ("A", L1, LTS), ("B", L1, LTS), ("C", L1, RBF), ("A", PEARSON, RBF)],
                         ids=["A-l1-rbf", "A-l1-lts", "B-l1-lts", "C-l1-rbf", "A-pearson-rbf"])
def test_repeatable_and_blind_to_the_padding_bitwise(shape, dist, gate):
    """two runs are bitwise equal, and so is a run on a batch whose padding holds other values: nothing past n_b is read into a result"""
    dev = _dev()
    inp = _inputs(shape)
    first, again = _hip(dev, shape, dist, gate), _hip(dev, shape, dist, gate)
    x = inp["x"].clone()
    g = torch.Generator().manual_seed(99)
    for b, n in enumerate(inp["lengths"]):
        x[b, n:] = 50.0 * torch.randn(x.shape[1] - n, x.shape[2], generator=g, dtype=torch.float64)
    other = _hip(dev, shape, dist, gate, x=x)
    for name, run in (("second run", again), ("other padding", other)):
        for k in ("xn", "P", "D", "t"):
            assert torch.equal(first[k], run[k]), f"{name}: {k} differs"
        for k in ("gw", "gt"):
            assert len(first[k]) == len(run[k])
            for g_, (a, b) in enumerate(zip(first[k], run[k])):
                assert torch.equal(a, b), f"{name}: {k}[{g_}] differs"


def test_nine_group_bank_equals_its_groups():
    """more groups than one *_bank call takes: the regate runs group by group, and every group's columns and gradients are those of
    the group run as a bank of its own"""
    dev = _dev()
    ops = _ops()
    inp = _inputs("A")
    C = SHAPES["A"]["C"]
    G = ops.BANK_MAX_GROUPS + 1
    g = torch.Generator().manual_seed(9)
    Ks, Ls = [1 + i % 3 for i in range(G)], [8 + 4 * i for i in range(G)]          # L = 8 .. 40: every edge of shape A's lengths
    ws = [torch.randn(K, C, L, generator=g) for K, L in zip(Ks, Ls)]
    r = torch.randn(SHAPES["A"]["B"], sum(Ks) * C, generator=g).to(dev)
    x = inp["x"].float().to(dev)
    lengths = torch.tensor(inp["lengths"], dtype=torch.int32, device=dev)
    xn = ops.instance_norm_len(x, lengths)
    for gate in (RBF, LTS):
        thrs = [torch.rand(1, K, C, generator=g) for K in Ks] if gate == LTS else None

        def run(idx, cols):
            wd = [ws[i].to(dev).requires_grad_(True) for i in idx]
            td = [thrs[i].to(dev).requires_grad_(True) for i in idx] if thrs else None
            P, D, t = ops.shapelet_bank(xn, wd, EPS, L1 | gate, [1] * len(idx), td, return_tstar=True, lengths=lengths)
            (P * r[:, cols]).sum().backward()
            return P.detach(), D, t, [w.grad for w in wd], [t_.grad for t_ in (td or [])]

        P, D, t, gw, gt = run(list(range(G)), slice(None))
        assert (t == -1).any() and (t >= 0).any()
        col = 0
        for i in range(G):
            cols = slice(col, col + Ks[i] * C)
            Pi, Di, ti, gwi, gti = run([i], cols)
            assert torch.equal(P[:, cols], Pi) and torch.equal(D[:, cols], Di) and torch.equal(t[:, cols], ti), f"group {i}"
            _grad_close(f"9 groups gate {gate:#x} grad_w[{i}]", gw[i], gwi[0])
            if gate == LTS:
                _grad_close(f"9 groups gate {gate:#x} grad_thr[{i}]", gt[i], gti[0])
            col += Ks[i] * C


def test_lengths_with_an_input_gradient_are_refused_at_forward_time():
    dev = _dev()
    ops = _ops()
    from ign_hip._lib import IgnError
    inp = _inputs("A")
    lengths = torch.tensor(inp["lengths"], dtype=torch.int32, device=dev)
    x = inp["x"].float().to(dev).requires_grad_(True)
    with pytest.raises(IgnError, match="length-aware ign_instnorm_bwd"):
        ops.instance_norm_len(x, lengths)
    xn = ops.instance_norm_len(x.detach(), lengths).requires_grad_(True)
    with pytest.raises(IgnError, match="length-aware ign_instnorm_bwd"):
        ops.shapelet_bank(xn, [inp["ws"][0].float().to(dev)], EPS, L1 | RBF, [1], None, lengths=lengths)


# ---------------------------------------------------------------------------------------------------------------- models
MODEL_KS, MODEL_FRACS = [3, 2], [0.08, 0.41]            # ceil(0.08 * 96) = 8, ceil(0.41 * 96) = 40: the groups of shape A


def _model_cfg(**kw):
    s = SHAPES["A"]
    return make_cfg(enc_in=s["C"], seq_len=s["T"], num_class=4, c_out=4, dec_in=s["C"], mask_padding=True, **kw)


def _keep_mask(lengths, T, dev):
    return (torch.arange(T).unsqueeze(0) < torch.tensor(lengths).unsqueeze(1)).float().to(dev)


def _oracle_model_features(ref_sbm, x, lengths, lts):
    """the oracle's shapelet groups, sample by sample on x[b, :n_b] -> P (B,F) with graph, Dmin, t*, gap"""
    ws = [s.weights for s in ref_sbm.shapelets]
    thrs = [s.threshold for s in ref_sbm.shapelets] if lts else [None] * len(ws)
    strides = [s.stride for s in ref_sbm.shapelets]
    rows = [_oracle_sample(x[b:b + 1, :n], ws, thrs, strides, L1, LTS if lts else RBF) for b, n in enumerate(lengths)]
    return tuple(torch.stack(f) for f in zip(*rows))


@pytest.mark.parametrize("name", ["SBM", "LTS", "InterpGN"])
def test_masked_models_match_the_per_sample_oracle(name):
    """ModelInfo (p, d, t, logits) of the masked model and the parameter gradients after one loss.backward(), against the oracle's
    modules in float64 fed sample by sample; the FCN expert of InterpGN sees the padded batch on both sides."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    from models.InterpGN import InterpGN
    from models.Shapelet import DistThresholdSBM, ShapeBottleneckModel
    from oracle import ign_oracle as O
    NO_WINDOW = _ops().NO_WINDOW
    inp, s = _inputs("A"), SHAPES["A"]
    lts = name == "LTS"
    cfg = _model_cfg()
    torch.manual_seed(11)
    if name == "InterpGN":
        ref = O.OracleIGN(cfg, num_shapelet=MODEL_KS, shapelet_len=MODEL_FRACS, chunk=64)
        model = InterpGN(cfg, num_shapelet=MODEL_KS, shapelet_len=MODEL_FRACS)
    else:
        ref = O.OracleSBM(cfg, num_shapelet=MODEL_KS, shapelet_len=MODEL_FRACS, lts=lts, chunk=64)
        model = (DistThresholdSBM if lts else ShapeBottleneckModel)(cfg, num_shapelet=MODEL_KS, shapelet_len=MODEL_FRACS)
    ref_sbm = ref.sbm if name == "InterpGN" else ref
    with torch.no_grad():                                # shape A's shapelets (the t* gap of the recipe holds for them)
        for sh, w in zip(ref_sbm.shapelets, inp["ws"]):
            sh.weights.copy_(w.float())
    model.load_state_dict(ref.state_dict())
    model.to(dev).train()
    ref.double().train()
    assert [sh.length for sh in (model.sbm if name == "InterpGN" else model).shapelets] == list(s["L"])
    x, lengths = inp["x"], inp["lengths"]
    y = torch.arange(s["B"]) % 4

    P, D, t, gap = _oracle_model_features(ref_sbm, x, lengths, lts)
    sbm_out = ref_sbm.output_layer(P)
    if name == "InterpGN":
        deep_out = ref.deep_model(x)
        out_r, _ = O.gini_gate(sbm_out, deep_out)
        info_r = O.OracleInfo(shapelet_preds=sbm_out, loss=ref_sbm.loss().unsqueeze(0))
    else:
        out_r, info_r = sbm_out, O.OracleInfo(shapelet_preds=sbm_out, loss=ref_sbm.loss().unsqueeze(0))
    O.train_loss(name, out_r, info_r, y).backward()

    out, info = model(x.float().to(dev), _keep_mask(lengths, s["T"], dev), None, None)
    loss = torch.nn.functional.cross_entropy(out, y.to(dev)) + info.loss.mean()
    if name == "InterpGN":
        loss = loss + torch.nn.functional.cross_entropy(info.shapelet_preds, y.to(dev))
    loss.backward()

    empty = t < 0
    assert empty.any()
    p_, d_, t_ = info.p.detach().cpu(), info.d.cpu(), info.t.cpu().long()
    assert (p_[empty] == 0).all() and (d_[empty] == np.float32(NO_WINDOW)).all() and (t_[empty] == -1).all()
    parity(f"{name} p", p_, P, tol=1e-4, kind="elem")
    parity(f"{name} d", d_[~empty], D[~empty], tol=1e-4, kind="elem")
    assert float(gap[~empty].min()) > 1e-4
    assert torch.equal(t_[~empty], t[~empty])
    parity(f"{name} logits", out, out_r, tol=1e-4, kind="elem")
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if n.startswith("deep_model.block") and n.endswith(".0.bias"):
            # a convolution bias in front of a batch-statistics BatchNorm has an identically zero gradient (as in smoke())
            assert float(p.grad.abs().max()) <= 1e-6 and float(q.grad.abs().max()) <= 1e-6, n
            continue
        assert p.grad is not None and q.grad is not None, n
        _grad_close(f"{name} grad {n}", p.grad, q.grad)


def test_mask_off_or_no_mask_is_the_unmasked_model():
    """the switch is opt-in: without it (or without a mask) the padded batch runs exactly as before, bit for bit"""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    from models.Shapelet import ShapeBottleneckModel
    inp, s = _inputs("A"), SHAPES["A"]
    x = inp["x"].float().to(dev)
    mask = _keep_mask(inp["lengths"], s["T"], dev)
    torch.manual_seed(3)
    on = ShapeBottleneckModel(_model_cfg(), num_shapelet=MODEL_KS, shapelet_len=MODEL_FRACS).to(dev).eval()
    cfg_off = _model_cfg()
    cfg_off.mask_padding = False
    off = ShapeBottleneckModel(cfg_off, num_shapelet=MODEL_KS, shapelet_len=MODEL_FRACS).to(dev).eval()
    off.load_state_dict(on.state_dict())
    with torch.no_grad():
        base = off(x)[1]
        for info in (off(x, mask)[1], on(x)[1], on(x, None)[1]):
            assert torch.equal(info.p, base.p) and torch.equal(info.d, base.d) and torch.equal(info.t, base.t)
        masked = on(x, mask)[1]
    assert not torch.equal(masked.p, base.p) and (masked.t == -1).any()


# ---------------------------------------------------------------------------------------------------------------- the reference itself
def test_masked_sbm_matches_the_reference_on_truncated_samples():
    """tests/golden/sbm_masked.npz: the reference's ShapeBottleneckModel run on x[b:b+1, :n_b] of the shape-A samples with
    n_b >= 40 (tests/golden/make_golden_masked.py) against ONE masked forward / backward over the padded batch"""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    from models.Shapelet import ShapeBottleneckModel
    g = golden("sbm_masked")
    model = ShapeBottleneckModel(_model_cfg(), num_shapelet=MODEL_KS, shapelet_len=MODEL_FRACS)
    model.load_state_dict(sd_from(g))
    model.to(dev).eval()
    x = torch.from_numpy(g["x"]).to(dev)
    lengths = [int(n) for n in g["lengths"]]
    _, info = model(x, _keep_mask(lengths, x.shape[1], dev))
    (info.p * torch.from_numpy(g["r"]).to(dev)).sum().backward()
    parity("reference p", info.p, g["p"], tol=1e-4, kind="elem")
    parity("reference d", info.d, g["d"], tol=1e-4, kind="elem")
    for i, sh in enumerate(model.shapelets):
        _grad_close(f"reference grad shapelets.{i}.weights", sh.weights.grad, g[f"grad.shapelets.{i}.weights"])


# ---------------------------------------------------------------------------------------------------------------- the driver
def test_harness_on_a_ragged_set_never_locates_a_match_in_the_padding(tmp_path, monkeypatch, capsys):
    """run.py's Experiment on a generated ragged .ts set (lengths 7..29 at T = 29, as JapaneseVowels) with --mask_padding: trains
    eagerly although --hipgraph is given, and in test() every located match lies inside its sample; a sample shorter than a
    shapelet reports t = -1, match_start = -1, match_len = 0, d = 0 (finite score).  Without the flag the same data does put
    matches into the padding, which is the defect the switch exists for."""
    _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    import run
    from data_provider.ts_reader import write_ts
    from exp.experiment_classification import Experiment, compute_shapelet_score
    d = tmp_path / "Rag"
    d.mkdir()
    classes = ["a", "b", "c"]
    lens = {}
    for split, seed in (("TRAIN", 1), ("TEST", 2)):
        rng = np.random.RandomState(seed)
        n = [29, 7] + [int(v) for v in rng.randint(7, 30, size=22)]
        X = [rng.randn(4, m) + np.sin(np.arange(m) * (1 + i % 3))[None, :] for i, m in enumerate(n)]
        write_ts(str(d / f"Rag_{split}.ts"), X, [classes[i % 3] for i in range(len(n))], "Rag", classes)
        lens[split] = n
    monkeypatch.chdir(tmp_path)
    beyond = {}
    for flag in (True, False):
        argv = ["--model", "SBM", "--data", "UEA", "--data_root", str(tmp_path), "--dataset", "Rag", "--train_epochs", "2",
                "--batch_size", "8", "--seed", "0", "--amp", "--num_shapelet", "2"] + (["--mask_padding", "--hipgraph"] if flag else [])
        run.set_seed(0)
        e = Experiment(run.get_args(argv))
        assert e.args.seq_len == 29
        e.train()
        _, res, _ = e.test(save_csv=False)
        n = torch.tensor(lens["TEST"]).unsqueeze(1)
        assert res.t.shape[0] == len(lens["TEST"])
        stride, length = e.model.match_layout()
        short = n < length.unsqueeze(0)                         # (N,F): the sample is shorter than the shapelet
        located = res.t >= 0
        end = res.match_start + (res.match_len if res.match_len.dim() == 2 else res.match_len.unsqueeze(0))
        beyond[flag] = int(((end > n) & located).sum())
        if flag:
            assert "--hipgraph ignored" in capsys.readouterr().out
            assert short.any() and torch.equal(~located, short)
            assert (res.match_start[short] == -1).all() and (res.match_len[short] == 0).all() and (res.d[short] == 0).all()
            assert torch.isfinite(res.d).all() and (res.p[short] == 0).all()
            score = compute_shapelet_score(res.d.float(), res.w.float(), res.preds, res.trues)
            assert np.isfinite(score) or not bool((res.preds == res.trues).any())
    assert beyond[True] == 0 and beyond[False] > 0
