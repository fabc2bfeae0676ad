"""bf16 autocast (the reference's default mode, the harness's too unless --amp is given): the single-product kernels of the dense
layers (GEMM_BF16: ign_clconv_fwd_bf16, ign_linear_wgrad_bf16, ign_clconv_wgrad_bf16) and of the attention core (ATTN_MATH_BF16:
ign_attn_fwd_bf16 / ign_attn_bwd_bf16) against float64 models that round every operand where the kernels round it.

A bf16 x bf16 product is exact in fp32, so a single-product GEMM equals the float64 GEMM of its operands rounded to bf16 (round to
nearest even: `tensor.bfloat16()`) up to the order of the fp32 accumulation.  Bounds (parts 1 - 3): 3e-6 for outputs and input
gradients, 1e-5 for weight and bias gradients -- those of test_gpu_fcn.py and test_linear_on_own_gemm_kernels: fp32 accumulation
stays within 3e-7 of the rounded model at these shapes, the unrounded float64 result is 1e-3 .. 3e-3 away.  The attention core also
rounds intermediates (P, dS); its bound is measured on the model alone (ATTN_*, tests/diag_bf16_parity.py).

Every comparison is printed and recorded (measured distance, the bound it is held to, distance of the unrounded float64 result);
with IGN_BF16_PARITY_OUT=<file> the record is written there as JSON when the module finishes.  The copy judged is
profiles/bf16_parity.json."""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from test_gpu_baselines import _dev, _rel
from test_gpu_fcn import _RoundedConv, _bf16r

pytestmark = pytest.mark.gpu

OUT_TOL, WGRAD_TOL = 3e-6, 1e-5          # outputs / input gradients; weight / bias gradients
NOT_EXACT = 1e-4                         # the unrounded float64 result must be further than this: the single-product kernel ran
_LEDGER = {}


@pytest.fixture(scope="module", autouse=True)
def _write_ledger():
    yield
    path = os.environ.get("IGN_BF16_PARITY_OUT")
    if not _LEDGER or not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(dict(bounds=dict(output=OUT_TOL, weight_gradient=WGRAD_TOL, not_exact=NOT_EXACT, attention=ATTN_TOL,
                                   attention_rms=ATTN_TOL_RMS),
                       cases=_LEDGER), f, indent=1, sort_keys=True)


class _Case:
    """The comparisons of one test case: each is printed and recorded before anything is asserted."""

    def __init__(self, name):
        self.name, self.bad = name, []
        self.rec = _LEDGER.setdefault(name, {})

    def hold(self, what, got, model, bound, exact=None, metric=_rel):
        """got within `bound` of the rounded-operand model; `exact`: the unrounded float64 result, its distance recorded."""
        d = metric(got, model)
        r = dict(rel=d, bound=bound)
        if exact is not None:
            r["unrounded_rel"] = metric(got, exact)
        self.rec[what] = r
        print(f"{self.name}: {what} {r}")
        if not d < bound:
            self.bad.append((what, r))
        return r

    def not_exact(self, what):
        """the recorded distance of `what` to the unrounded float64 result is beyond NOT_EXACT"""
        if not self.rec[what]["unrounded_rel"] > NOT_EXACT:
            self.bad.append((what + " equals the unrounded result", self.rec[what]))

    def finish(self):
        assert not self.bad, f"{self.name}: {self.bad}"


def _ops():
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import _lib, ops
    return _lib, ops


def _autocast():
    return torch.autocast(device_type="cuda", dtype=torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------ 1. ops.linear
def _linear_model(x, w, b, gy, split):
    """float64 on the CPU.  -> (model, exact): y = r(x) r(w)^T + b, dx = r(gy) r(w), dW = r(gy)^T r(x) on the split kernel and
    gy^T x (unrounded) on the fp32 kernel, db = column sums of the UNROUNDED gy (ign_linear_wgrad_bf16 accumulates them before it
    forms the bf16 plane; the fp32 route sums gy itself)."""
    Ci, Co = w.shape[1], w.shape[0]
    x2, g2, wd = x.double().reshape(-1, Ci), gy.double().reshape(-1, Co), w.double()
    xr, gr, wr = _bf16r(x).reshape(-1, Ci), _bf16r(gy).reshape(-1, Co), _bf16r(w)
    bd = b.double() if b is not None else torch.zeros(Co, dtype=torch.float64)
    exact = dict(y=(x2 @ wd.t() + bd).reshape(gy.shape), dx=(g2 @ wd).reshape(x.shape), dW=g2.t() @ x2, db=g2.sum(0))
    model = dict(y=(xr @ wr.t() + bd).reshape(gy.shape), dx=(gr @ wr).reshape(x.shape), dW=gr.t() @ xr if split else exact["dW"],
                 db=exact["db"])
    return model, exact


def _linear_inputs(shape, Co, bias):
    Ci = shape[-1]
    g = torch.Generator().manual_seed(7 * sum(shape) + Co)
    x = torch.randn(*shape, generator=g)
    w = torch.randn(Co, Ci, generator=g) / Ci ** 0.5
    b = torch.randn(Co, generator=g) if bias else None
    gy = torch.randn(*shape[:-1], Co, generator=g)
    return x, w, b, gy


def _check_linear(shape, Co, bias, tag=""):
    dev = _dev()
    _, ops = _ops()
    x, w, b, gy = _linear_inputs(shape, Co, bias)
    split = ops._linear_wgrad_split(shape[-1])
    model, exact = _linear_model(x, w, b, gy, split)
    xg, wg = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    bg = b.to(dev).requires_grad_(True) if bias else None
    with _autocast():
        y = ops.linear(xg, wg, bg)
    assert y.dtype == torch.float32
    (y * gy.to(dev)).sum().backward()
    c = _Case(f"linear{tag} {tuple(shape)}->{Co} bias={bias}")
    c.hold("y", y, model["y"], OUT_TOL, exact["y"])
    c.hold("dx", xg.grad, model["dx"], OUT_TOL, exact["dx"])
    c.hold("dW", wg.grad, model["dW"], WGRAD_TOL, exact["dW"])
    if bias:
        c.hold("db", bg.grad, model["db"], WGRAD_TOL)
    c.not_exact("y")
    c.not_exact("dx")
    if split:
        c.not_exact("dW")
    c.finish()
    return split


# (M, Ci, Co): one row, one staged float4 | less than a 16-row unit, Co % 4 only | two ci tiles and two co tiles whose second has 4
# live columns, ragged second unit | three co tiles | 33 units = 2 splits of 17 + 16, 11 live rows in the last unit | 257 units = 9
# splits: a second round over the 8 XCDs, 7 workgroups return early | Ci % 4 != 0: the weight gradient leaves the split kernel
_LINEAR_SHAPES = [(1, 4, 4), (15, 8, 12), (17, 132, 132), (129, 64, 260), (523, 128, 64), (4100, 64, 64), (5, 130, 12)]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("M,Ci,Co", _LINEAR_SHAPES)
def test_linear_inside_autocast_equals_rounded_operand_products(M, Ci, Co, bias):
    """ops.linear inside autocast: fp32 output; y, dx and dW equal the float64 products of the bf16-rounded operands, db the column
    sums of the unrounded gy, and none of them is the unrounded float64 result.  Where the weight gradient leaves the split kernel
    (ops._linear_wgrad_split: Ci % 4 != 0, here (5, 130, 12)) it runs on the fp32 kernel, which does not round: the test takes its dW
    reference by the same predicate -- the present mixed arithmetic, recorded, not judged."""
    split = _check_linear((M, Ci), Co, bias)
    assert split == (Ci % 4 == 0)


def test_linear_inside_autocast_with_leading_dimensions():
    """(3, 43, 64) -> 32: the reshape of input and upstream gradient to rows, 129 rows."""
    assert _check_linear((3, 43, 64), 32, True)


def test_linear_inside_autocast_with_the_fp32_weight_gradient(monkeypatch):
    """LINEAR_WGRAD = "f32": forward and input gradient stay on the single-product kernels, dW = gy^T x unrounded (fp32 MFMA)."""
    _, ops = _ops()
    monkeypatch.setattr(ops, "LINEAR_WGRAD", "f32")
    assert not _check_linear((523, 128), 64, True, tag=" wgrad=f32")


# ---------------------------------------------------------------------------------------------------------- 3. gelu_linear
@pytest.mark.parametrize("shape,Ci,Co,bias", [((4, 300, 512), 512, 128, True), ((3, 77, 256), 256, 64, False), ((130, 64), 64, 12, True),
                                              ((2, 50, 768), 768, 256, True), ((15, 8), 8, 12, True)])
def test_gelu_linear_inside_autocast_equals_rounded_operand_products(shape, Ci, Co, bias):
    """ops.gelu_linear inside autocast.  a = F.gelu(u) in fp32 on the device enters the model as data (a float64 GELU would flip
    bf16 ties of a); z = r(a) r(w)^T + b, dL/du = gelu'(u) (r(gz) r(w)) with gelu' in float64, dW = r(gz)^T r(a), db = column sums
    of the unrounded gz.  The fused input-gradient kernel of the f16x3 arithmetic must not run here."""
    dev = _dev()
    _lib, ops = _ops()
    g = torch.Generator().manual_seed(Ci + Co)
    u = torch.randn(*shape, generator=g) * 1.5
    w = torch.randn(Co, Ci, generator=g) / Ci ** 0.5
    b = torch.randn(Co, generator=g) * 0.1 if bias else None
    gz = torch.randn(*shape[:-1], Co, generator=g)
    ug, wg = u.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    bg = b.to(dev).requires_grad_(True) if bias else None
    L = _lib.lib()
    fused_calls = []
    orig = L.ign_linear_dgrad_gelu_h3
    L.ign_linear_dgrad_gelu_h3 = lambda *a: (fused_calls.append(1), orig(*a))[1]
    try:
        with _autocast():
            z = ops.gelu_linear(ug, wg, bg)
        assert z.dtype == torch.float32
        (z * gz.to(dev)).sum().backward()
    finally:
        L.ign_linear_dgrad_gelu_h3 = orig
    assert not fused_calls
    a = F.gelu(u.to(dev)).cpu()
    split = ops._linear_wgrad_split(Ci)
    assert split
    model, _ = _linear_model(a, w, b, gz, split)
    ud, wd = u.double().requires_grad_(True), w.double().requires_grad_(True)
    dgelu, = torch.autograd.grad(F.gelu(ud).sum(), ud)
    zd = F.linear(F.gelu(ud), wd, b.double() if bias else None)
    (zd * gz.double()).sum().backward()
    c = _Case(f"gelu_linear {tuple(shape)}->{Co} bias={bias}")
    c.hold("z", z, model["y"], OUT_TOL, zd)
    c.hold("du", ug.grad, dgelu * model["dx"], OUT_TOL, ud.grad)
    c.hold("dW", wg.grad, model["dW"], WGRAD_TOL, wd.grad)
    if bias:
        c.hold("db", bg.grad, model["db"], WGRAD_TOL)
    for what in ("z", "du", "dW"):
        c.not_exact(what)
    c.finish()


# ------------------------------------------------------------------------------------------------------------ 3. conv1d_cl
@pytest.mark.parametrize("B,Tin,Ci,Co,k,bias,route", [(3, 40, 6, 64, 3, False, "split"), (2, 130, 12, 64, 4, True, "taps"),
                                                      (4, 27, 64, 128, 3, False, "split"), (2, 300, 122, 512, 3, False, "split"),
                                                      (1, 17, 5, 8, 7, True, "f32"), (2, 64, 128, 128, 1, True, "f32"),
                                                      (3, 33, 7, 12, 11, False, "f32")])
def test_conv1d_cl_inside_autocast_equals_rounded_operand_products(B, Tin, Ci, Co, k, bias, route):
    """ops.conv1d_cl inside autocast on the three weight-gradient routes of ops._conv_wgrad_route -- "split" (the multi-tap kernel),
    "taps" (one ign_linear_wgrad_bf16 per tap on row views advanced by j rows), "f32" (ign_clconv_wgrad: no rounding) -- against
    _RoundedConv, the float64 algebra of test_gpu_fcn.py: y, dx and (split, taps) dW from the bf16-rounded operands, the "f32"
    route's dW from the unrounded ones, db = sums of the unrounded gy.  The route each shape takes is asserted."""
    dev = _dev()
    _, ops = _ops()
    assert ops._conv_wgrad_route(k, Ci) == route
    g = torch.Generator().manual_seed(B * 1000 + Tin + Ci + Co + k)
    x = torch.randn(B, Tin, Ci, generator=g)
    w = torch.randn(Co, Ci, k, generator=g) / (Ci * k) ** 0.5
    b = torch.randn(Co, generator=g) if bias else None
    gy = torch.randn(B, Tin - k + 1, Co, generator=g)
    xg, wg = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    bg = b.to(dev).requires_grad_(True) if bias else None
    with _autocast():
        y = ops.conv1d_cl(xg, wg, bg)
    assert y.dtype == torch.float32
    (y * gy.to(dev)).sum().backward()
    # the unrounded float64 convolution, and the rounded-operand model
    xe, we = x.double().requires_grad_(True), w.double().requires_grad_(True)
    be = b.double().requires_grad_(True) if bias else None
    ye = F.conv1d(xe.permute(0, 2, 1), we, be).permute(0, 2, 1)
    (ye * gy.double()).sum().backward()
    xm, wm = x.double().requires_grad_(True), w.double().requires_grad_(True)
    bm = (b.double() if bias else torch.zeros(Co, dtype=torch.float64)).requires_grad_(True)
    ym = _RoundedConv.apply(xm.permute(0, 2, 1), wm, bm).permute(0, 2, 1)
    (ym * gy.double()).sum().backward()
    c = _Case(f"conv1d_cl B={B} Tin={Tin} Ci={Ci} Co={Co} k={k} bias={bias} route={route}")
    c.hold("y", y, ym, OUT_TOL, ye)
    c.hold("dx", xg.grad, xm.grad, OUT_TOL, xe.grad)
    c.hold("dW", wg.grad, we.grad if route == "f32" else wm.grad, WGRAD_TOL, we.grad)
    if bias:
        c.hold("db", bg.grad, bm.grad, WGRAD_TOL)
        assert torch.equal(bm.grad, be.grad)                  # the model's bias gradient is the unrounded sum
    c.not_exact("y")
    c.not_exact("dx")
    if route != "f32":
        c.not_exact("dW")
    c.finish()


# ------------------------------------------------------------------------------------------------------------ 4. attention
LOG2E = 1.4426950408889634
# Noise floor of the model below (tests/diag_bf16_parity.py --noise-floor, CPU only, recorded in profiles/bf16_parity.json): the
# model run twice per shape, the second time with every intermediate that an fp32 kernel forms in front of a bf16 rounding point
# moved by a relative 2^-23 (random sign, seed 0); the largest distance between the two runs over out, dq, dk, dv and the five
# shapes.  An fp32 value within rounding of a bf16 tie rounds the other way than its float64 twin, which moves that operand by 2^-8
# of its value.  ATTN_FACTOR covers the accumulation order and an exp2 of a few ulp.
#   _rel (largest element error over the largest element): noise 1.166e-3 -> bound 4.66e-3.  One flipped probability of a dominant
#     key shows in full, so this bound is NOT 10x below the model's distance to the unrounded float64 attention (2e-3 .. 2e-2 in
#     _rel): on its own it proves little more than test_attention_inside_autocast_is_the_bf16_single_product_form (3e-2 / 5e-2
#     against the unrounded result), which stays as it is.
#   _rms_rel (root mean square error over the root mean square): the flips are sparse, so the same two runs differ by 1.163e-4 at
#     most -> bound 4.65e-4, 3.6x (the one-key shape) to 13x below the distance to the unrounded result (1.7e-3 .. 6e-3) and below
#     what a misplaced rounding point costs in at least one quantity (P rounded after normalisation: out 2e-3; delta or dP from the
#     other form of dO: dq, dk 7e-4 .. 3e-3; the row sum from the rounded p: dq, dk, dv 6e-4 .. 1.2e-3; dS left unrounded: 1.6e-3;
#     the dK / dV score with the factor on q: dk, dv 4e-3 -- each measured by editing the model, tests/diag_bf16_parity.py).
# The kernels on the MI355X (profiles/bf16_parity.json): 3.2e-4 at most in _rel, 3.9e-5 in _rms_rel; 1e-7 where no tie flips.
ATTN_NOISE, ATTN_NOISE_RMS = 1.166e-3, 1.163e-4
ATTN_FACTOR = 4.0
ATTN_TOL, ATTN_TOL_RMS = ATTN_FACTOR * ATTN_NOISE, ATTN_FACTOR * ATTN_NOISE_RMS


def _rms_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).square().mean().sqrt() / b.square().mean().sqrt().clamp_min(1e-12))


_ATTN_SHAPES = [(2, 200, 200, 4, 64), (2, 130, 75, 2, 32), (1, 33, 257, 3, 16), (1, 1, 1, 1, 16), (1, 31, 33, 2, 64)]


def _attn_inputs(B, L, S, H, E):
    g = torch.Generator().manual_seed(L + S + E)
    q = torch.randn(B, L, H, E, generator=g)
    k = torch.randn(B, S, H, E, generator=g)
    v = torch.randn(B, S, H, E, generator=g)
    go = torch.randn(B, L, H, E, generator=g)
    return q, k, v, go


def _attn_exact(q, k, v, go, scale):
    """softmax(scale Q K^T) V and its three gradients in float64, nothing rounded."""
    qr, kr, vr = (t.detach().double().cpu().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("blhe,bshe->bhls", qr, kr)
    o = torch.einsum("bhls,bshd->blhd", torch.softmax(scale * s, dim=-1), vr)
    (o * go.double()).sum().backward()
    return dict(out=o.detach(), dq=qr.grad, dk=kr.grad, dv=vr.grad)


def _attn_model(q, k, v, go, scale, pre=lambda t: t):
    """float64 restatement of ign_attn_fwd_bf16 / ign_attn_bwd_bf16 (csrc/ign_attention_x6.hip, plane count 1), r() = round to bf16
    through fp32.  `pre` is applied to every intermediate that the kernels hold in fp32 in front of a rounding point (identity for
    the model; the noise-floor measurement perturbs there).  c = fp32(scale) * fp32(log2 e); scores are in base 2.

    forward (attn_fwd_x6_kernel): S = r(q c) . r(k) -- the fp32 product q c is rounded, k as it is staged.  Keys go in blocks of 32
    with a running row maximum m: p = exp2(S - m) is NOT normalised when it is rounded; the row sum l is taken from the UNROUNDED p;
    O = O exp2(m_old - m) + r(p) r(v); out = O / l at the end; lse = m ln 2 + ln l.
    delta = rowsum(dO * out) from the unrounded fp32 dO and out (attn_bwd_dq_x6_kernel, read again by the dK kernel).
    dQ (attn_bwd_dq_x6_kernel): S as in the forward; dP = r(dO) . r(v); P = exp2(S - lse log2 e), normalised, not rounded on its own;
    dS = P (dP - delta) in fp32, rounded; dQ = scale * r(dS) r(k) -- the scale once at the end, k unscaled.
    dK, dV (attn_bwd_dkv_x6_kernel): the score is recomputed with the factor on the OTHER operand, S' = r(q) . r(k c); P' = exp2(S' -
    lse log2 e); dV = r(P')^T r(dO); dP = r(dO) . r(v); dS' = P' (dP - delta) rounded; dK = scale * r(dS')^T r(q)."""
    r = _bf16r
    qf, kf, vf, gf = (t.detach().float().cpu() for t in (q, k, v, go))
    sc32 = torch.tensor(scale, dtype=torch.float32)
    c = sc32 * torch.tensor(LOG2E, dtype=torch.float32)
    qs, ks = r(pre((qf * c).double())), r(pre((kf * c).double()))
    qr, kr, vr, gr = r(qf), r(kf), r(vf), r(gf)
    S2 = pre(torch.einsum("blhe,bshe->bhls", qs, kr))
    B, H, L, S = S2.shape
    m = torch.full((B, H, L), -math.inf, dtype=torch.float64)
    l = torch.zeros(B, H, L, dtype=torch.float64)
    O = torch.zeros(B, H, L, qf.shape[-1], dtype=torch.float64)
    for s0 in range(0, S, 32):
        blk = S2[..., s0:s0 + 32]
        mn = torch.maximum(m, blk.amax(-1))
        alpha = torch.exp2(m - mn)
        p = pre(torch.exp2(blk - mn[..., None]))
        l = l * alpha + p.sum(-1)
        O = O * alpha[..., None] + torch.einsum("bhls,bshd->bhld", r(p), vr[:, s0:s0 + 32])
        m = mn
    out = (O / l[..., None]).permute(0, 2, 1, 3)                             # (B, L, H, E)
    lse2 = pre(m + torch.log2(l))[..., None]
    delta = pre((gf.double() * out).sum(-1)).permute(0, 2, 1)[..., None]      # (B, H, L, 1)
    scale = float(sc32)
    dS = pre(pre(torch.exp2(S2 - lse2)) * (pre(torch.einsum("blhd,bshd->bhls", gr, vr)) - delta))
    dq = scale * torch.einsum("bhls,bshe->blhe", r(dS), kr)
    Pb = pre(torch.exp2(pre(torch.einsum("blhe,bshe->bhls", qr, ks)) - lse2))
    dv = torch.einsum("bhls,blhd->bshd", r(Pb), gr)
    dSb = pre(Pb * (pre(torch.einsum("blhd,bshd->bhls", gr, vr)) - delta))
    dk = scale * torch.einsum("bhls,blhe->bshe", r(dSb), qr)
    return dict(out=out, dq=dq, dk=dk, dv=dv)


def _fp32_noise(seed=0):
    """x -> x (1 +- 2^-23), the sign drawn per element from a seeded generator."""
    g = torch.Generator().manual_seed(seed)

    def pre(t):
        sign = torch.randint(0, 2, t.shape, generator=g, dtype=torch.int64) * 2 - 1
        return t * (1.0 + sign.double() * 2.0 ** -23)
    return pre


@pytest.mark.parametrize("B,L,S,H,E", _ATTN_SHAPES)
def test_attention_inside_autocast_equals_the_model_with_the_kernels_rounding_points(B, L, S, H, E):
    """ops.attention inside autocast against _attn_model (its docstring lists the rounding points): out, dq, dk, dv within
    ATTN_TOL in _rel and within ATTN_TOL_RMS in _rms_rel, both measured on the model alone (see the constants: only the second
    separates the rounding points); (1, 1, 1, 1, 16) and (1, 31, 33, 2, 64) are less than one tile in both directions.  The single
    softmax weight of (1, 1, 1, 1, 16) is 1 whatever the score: the output shows the rounding of v alone, and dq, dk -- exactly
    zero without rounding -- are what is left of dP - delta = (r(dO) - dO) . r(v)."""
    dev = _dev()
    _, ops = _ops()
    q, k, v, go = _attn_inputs(B, L, S, H, E)
    scale = 1.0 / math.sqrt(E)
    qg, kg, vg = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    with _autocast():
        o = ops.attention(qg, kg, vg, scale)
    assert o.dtype == torch.float32
    (o * go.to(dev)).sum().backward()
    model, exact = _attn_model(q, k, v, go, scale), _attn_exact(q, k, v, go, scale)
    c = _Case(f"attention B={B} L={L} S={S} H={H} E={E}")
    for what, got in (("out", o), ("dq", qg.grad), ("dk", kg.grad), ("dv", vg.grad)):
        c.hold(what, got, model[what], ATTN_TOL, exact[what])
        c.hold(what + " rms", got, model[what], ATTN_TOL_RMS, exact[what], metric=_rms_rel)
    c.not_exact("out")
    c.finish()
