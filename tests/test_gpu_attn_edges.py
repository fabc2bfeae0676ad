"""The attention kernels at every tile edge and in sharp-softmax rows (tests/attn_edge_cases.py holds the tables, the geometry and
the bounds; tests/test_attn_edges_host.py proves what the tables cover): every (arithmetic, head width) route against float64 at
the 16 (L, S) pairs of the edge table, forward, backward and map; dropout and the packed entry point at the edges; the exported
split backward at E = 128 that `ops` never routes to; seven score regimes whose softmax rows are sharp, monotone, tied, uniform;
and the operand views the wrapper has to copy.

The three fp32-accurate routes are judged slice by slice (attn_edge_cases.slice_err) against the float64 formula; the bf16 route
against the rounded-operand model of tests/test_gpu_bf16_parity.py with that file's metrics and bounds.  Every figure is printed
and recorded before anything is asserted; IGN_ATTN_EDGES_OUT=<file> writes the record as JSON when the module finishes
(tests/diag_attn_edges.py -> profiles/attn_edges.json)."""
import contextlib
import ctypes
import json
import os

import pytest
import torch

import attn_edge_cases as C
from test_attn_dropout_host import dropout_threshold
from test_gpu_attn_dropout import _Seeds, _dev, _mod, _ref_dropout_attention, device_mask
from test_gpu_attn_map import _ref_probs
from test_gpu_bf16_parity import ATTN_TOL, ATTN_TOL_RMS

pytestmark = pytest.mark.gpu

_RECORD = {}
TENSORS = ("out", "dq", "dk", "dv")


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("IGN_ATTN_EDGES_OUT")
    if not _RECORD or not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(_RECORD, f, indent=1, sort_keys=True)


class _Case:
    """The comparisons of one case: each is printed and recorded before anything is asserted."""

    def __init__(self, section, name):
        self.name, self.bad = f"{section} {name}", []
        self.rec = _RECORD.setdefault(section, {}).setdefault(name, {})

    def hold(self, what, err, tol, **more):
        r = dict(err=err, tol=tol, ratio=(err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))), **more)
        self.rec[what] = r
        print(f"{self.name}: {what} {r}")
        if not err <= tol:
            self.bad.append((what, r))

    def finish(self):
        assert not self.bad, f"{self.name}: {self.bad}"


def _select(monkeypatch, ops, amath, E):
    """set the knobs of the arithmetic, check that the route is the one the tables mean, -> the context the call runs in"""
    attn_math, gemm_math, autocast = C.knobs(amath)
    monkeypatch.setattr(ops, "ATTN_MATH", attn_math)
    monkeypatch.setattr(ops, "GEMM_MATH", gemm_math)
    assert (ops._attn_arith(E, autocast, False, True), ops._attn_arith(E, autocast, True)) == C.route_arith(amath, E)
    assert ops._attn_arith(E, autocast, False, False) == C.inference_arith(amath, E)
    return torch.autocast(device_type="cuda", dtype=torch.bfloat16) if autocast else contextlib.nullcontext()


def _hold_inference_forward(c, ops, ctx, amath, E, inputs, scale, dev, ref_out, tol):
    """where a call that is not differentiated runs another forward kernel than one that is (E = 128 under the split arithmetics:
    attn_fwd_x6_kernel<128> against the fp32-MFMA pair), that forward too"""
    if C.inference_arith(amath, E) == C.route_arith(amath, E)[0]:
        return
    q, k, v, _ = inputs
    with ctx, torch.no_grad():
        out = ops.attention(q.to(dev), k.to(dev), v.to(dev), scale)
    c.hold("out (not differentiated)", C.slice_err(out, ref_out), tol)


def _run(ops, ctx, inputs, scale, dev, **kw):
    """ops.attention forward and backward under dO -> dict(out, dq, dk, dv[, attn])"""
    q, k, v, go = inputs
    qg, kg, vg = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    with ctx:
        res = ops.attention(qg, kg, vg, scale, **kw)
    out, attn = res if isinstance(res, tuple) else (res, None)
    assert out.dtype == torch.float32 and out.shape == q.shape
    (out * go.to(dev)).sum().backward()
    got = dict(out=out.detach(), dq=qg.grad, dk=kg.grad, dv=vg.grad)
    assert got["dq"].shape == q.shape and got["dk"].shape == k.shape and got["dv"].shape == v.shape
    if attn is not None:
        got["attn"] = attn
    return got


def _hold_bf16(c, got, model, floors=None, tols=None):
    """the bf16 route against the rounded-operand model (C.bf16_model_err: the metrics of tests/test_gpu_bf16_parity.py).
    `floors`: gradients that are identically zero before rounding are judged against their natural scale, as the fp32-accurate
    routes' are.  At S = 1 the model's dq and dk are not zero but the rounding residue (r(dO) - dO) . r(v), about 1e-4 of that
    scale: there the comparison only says that the kernel returns something finite and no larger than the natural scale x the
    bound -- zeros would pass.  The residue itself is held to the model by tests/test_gpu_bf16_parity.py at (1, 1, 1, 1, 16); on
    these rows its own fp32 noise is 5 .. 37 x that file's rms bound, above any tolerance this file may set, so the distance
    relative to the model's own maximum is recorded (`of_model`), not asserted."""
    for what in TENSORS:
        floor = (floors or {}).get(what)
        tmax, trms = (tols or {}).get(what, (ATTN_TOL, ATTN_TOL_RMS))
        if floor == 0.0:
            tmax = trms = 0.0                                           # identically zero with a zero natural scale: exact zeros
        emax, erms = C.bf16_model_err(got[what], model[what], floor)
        more = {} if not floor else dict(of_model=C.bf16_model_err(got[what], model[what])[0])
        c.hold(what, emax, tmax, **more)
        c.hold(what + " rms", erms, trms)


_TABLE = [pytest.param(a, E, L, S, id=f"{a}-E{E}-L{L}-S{S}") for a, E in C.ROUTES for L, S in C.EDGE_PAIRS]


# ----------------------------------------------------------------------------------------------------------------- a. edge table
@pytest.mark.parametrize("amath,E,L,S", _TABLE)
def test_edge_table_vs_float64(amath, E, L, S, monkeypatch):
    dev = _dev()
    _, ops = _mod()
    ctx = _select(monkeypatch, ops, amath, E)
    inputs, scale = C.edge_inputs(L, S, E), C.scale_of(E)
    got = _run(ops, ctx, inputs, scale, dev)
    c = _Case("edge", f"{amath} E={E} L={L} S={S}")
    floors = C.zero_floors(*inputs, scale, S)
    if amath == "bf16":
        _hold_bf16(c, got, C.edge_bf16_model(L, S, E), floors)
    else:
        ref = C.edge_reference(L, S, E)
        for what in TENSORS:
            c.hold(what, C.slice_err(got[what], ref[what], floor=floors.get(what, 0.0)), C.FWD_TOL if what == "out" else C.GRAD_TOL)
        _hold_inference_forward(c, ops, ctx, amath, E, inputs, scale, dev, ref["out"], C.FWD_TOL)
    c.finish()


# ----------------------------------------------------------------------------------------------------------------- b. the map
@pytest.mark.parametrize("amath,E,L,S", _TABLE)
def test_edge_table_map_at_p0(amath, E, L, S, monkeypatch):
    dev = _dev()
    _, ops = _mod()
    ctx = _select(monkeypatch, ops, amath, E)                          # not differentiated: C.inference_arith
    q, k, v, _ = C.edge_inputs(L, S, E)
    B, H = C.batch_heads(E)
    with ctx, torch.no_grad():
        out, attn = ops.attention(q.to(dev), k.to(dev), v.to(dev), C.scale_of(E), need_weights=True)
    assert attn.shape == (B, H, L, S) and attn.dtype == torch.float32 and attn.is_contiguous()
    c = _Case("map", f"{amath} E={E} L={L} S={S}")
    c.hold("row sums", float((attn.double().sum(-1) - 1.0).abs().max()), C.MAP_ROWSUM_TOL)
    av = torch.einsum("bhls,bshd->blhd", attn.double().cpu(), v.double())
    if amath == "bf16":
        c.hold("map", C.whole_err(attn, _ref_probs(q, k, C.scale_of(E), bf16=True)), C.MAP_TOL["bf16"])
        c.hold("attn @ v", C.whole_err(out, av), C.MAP_OUT_TOL["bf16"])
    else:
        c.hold("map", C.slice_err(attn, C.edge_reference(L, S, E)["probs"], dims=(2, 3)), C.FWD_TOL)
        c.hold("attn @ v", C.slice_err(out, av), C.FWD_TOL)
    c.finish()


# ----------------------------------------------------------------------------------------------------------------- c. dropout
@pytest.mark.parametrize("amath,E,L,S", [pytest.param(a, E, L, S, id=f"{a}-E{E}-L{L}-S{S}")
                                         for a, E in C.ROUTES for L, S in C.DROPOUT_PAIRS])
def test_dropout_at_the_edges_with_the_dumped_mask(amath, E, L, S, monkeypatch):
    dev = _dev()
    _, ops = _mod()
    ctx = _select(monkeypatch, ops, amath, E)
    rec = _Seeds(monkeypatch, ops)
    p, scale = 0.5, C.scale_of(E)
    q, k, v, go = C.edge_inputs(L, S, E)
    B, H = C.batch_heads(E)
    got = _run(ops, ctx, (q, k, v, go), scale, dev, dropout_p=p)
    assert len(rec.seeds) == 1
    Z = device_mask(B, H, L, S, p, rec.seeds[0])
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    oref = _ref_dropout_attention(qr, kr, vr, scale, Z, dropout_threshold(p)[1])
    (oref * go.double()).sum().backward()
    ref = dict(out=oref.detach(), dq=qr.grad, dk=kr.grad, dv=vr.grad)
    c = _Case("dropout", f"{amath} E={E} L={L} S={S}")
    for what in TENSORS:
        if amath == "bf16":
            tol = C.BF16_DROPOUT_FWD_TOL if what == "out" else C.BF16_DROPOUT_GRAD_TOL
        else:
            tol = C.FWD_TOL if what == "out" else C.GRAD_TOL
        c.hold(what, C.whole_err(got[what], ref[what]), tol)
    c.finish()


@pytest.mark.parametrize("L,S", C.DROPOUT_PAIRS)
def test_dropout_forward_of_a_call_that_is_not_differentiated_at_E128(L, S, monkeypatch):
    """attn_fwd_x6_kernel<128, 3, DROPOUT>: a differentiated call at E = 128 runs the fp32-MFMA pair, so the dropout form of the
    split forward is reached without gradients only.  Output against float64 with the dumped mask, map against the masked
    float64 softmax."""
    dev = _dev()
    _, ops = _mod()
    E, p = 128, 0.5
    ctx = _select(monkeypatch, ops, "bf16x6", E)
    assert C.inference_arith("bf16x6", E) == C.ATTN_MATH_X6
    rec = _Seeds(monkeypatch, ops)
    q, k, v, _ = C.edge_inputs(L, S, E)
    B, H = C.batch_heads(E)
    with ctx, torch.no_grad():
        out, attn = ops.attention(q.to(dev), k.to(dev), v.to(dev), C.scale_of(E), dropout_p=p, need_weights=True)
    assert len(rec.seeds) == 1
    Z, s = device_mask(B, H, L, S, p, rec.seeds[0]), dropout_threshold(p)[1]
    c = _Case("dropout", f"bf16x6 E={E} L={L} S={S} (not differentiated)")
    c.hold("out", C.whole_err(out, _ref_dropout_attention(q.double(), k.double(), v.double(), C.scale_of(E), Z, s)), C.FWD_TOL)
    c.hold("map", C.whole_err(attn, C.edge_reference(L, S, E)["probs"] * Z.double() * float(s)), C.FWD_TOL)
    assert torch.equal(attn.cpu() == 0, ~Z), "exactly the dropped entries are 0"
    c.finish()


@pytest.mark.parametrize("amath", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("E", [16, 32, 64])
@pytest.mark.parametrize("n", C.PACKED_LENGTHS)
def test_packed_dropout_at_the_edges(n, E, amath, monkeypatch):
    """ops.attention_packed (gradients written through the strided backward) with L = S one past a wave and one past a workgroup:
    float64 with the dumped mask, and the unpacked call with the same seed -- bitwise under bf16x6 (under f16x3 the views share the
    packed tensor's bound, the copies have their own: tests/test_gpu_baselines.py, the packed test)."""
    dev = _dev()
    _, ops = _mod()
    _select(monkeypatch, ops, amath, E)
    rec = _Seeds(monkeypatch, ops)
    p, scale = 0.5, C.scale_of(E)
    q, k, v, go = C.edge_inputs(n, n, E)
    B, H = C.batch_heads(E)
    qkv = torch.stack([q, k, v], dim=2).to(dev).requires_grad_(True)
    torch.manual_seed(11)
    o1 = ops.attention_packed(qkv, scale, dropout_p=p)
    g1, = torch.autograd.grad(o1, qkv, go.to(dev))
    qg, kg, vg = (qkv[:, :, i].detach().contiguous().requires_grad_(True) for i in range(3))
    torch.manual_seed(11)
    o2 = ops.attention(qg, kg, vg, scale, dropout_p=p)
    g2 = torch.stack(torch.autograd.grad(o2, (qg, kg, vg), go.to(dev)), dim=2)
    assert len(rec.seeds) == 2 and rec.seeds[0] == rec.seeds[1]
    c = _Case("packed", f"{amath} E={E} L=S={n}")
    if amath == "bf16x6":
        assert torch.equal(o1, o2), "packed output differs from the unpacked call"
        assert torch.equal(g1, g2), "packed gradient differs from the unpacked call"
    else:
        c.hold("out vs unpacked", C.whole_err(o1, o2), 1e-6)
        c.hold("grad vs unpacked", C.whole_err(g1, g2), 1e-6)
    Z = device_mask(B, H, n, n, p, rec.seeds[0])
    qkv_r = qkv.detach().double().cpu().requires_grad_(True)
    oref = _ref_dropout_attention(qkv_r[:, :, 0], qkv_r[:, :, 1], qkv_r[:, :, 2], scale, Z, dropout_threshold(p)[1])
    gref, = torch.autograd.grad(oref, qkv_r, go.double())
    c.hold("out", C.whole_err(o1, oref), C.FWD_TOL)
    for i, what in enumerate(("dq", "dk", "dv")):
        c.hold(what, C.whole_err(g1[:, :, i], gref[:, :, i]), C.GRAD_TOL)
    c.finish()


# ----------------------------------------------------------------------------------------------------------------- d. unrouted
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("L,S", C.UNROUTED_PAIRS)
def test_exported_split_backward_at_E128(L, S, strided):
    """ign_attn_bwd_x6 and ign_attn_bwd_x6_strided at E = 128 (exported, reachable through the C ABI, never chosen by ops: the
    fp32-MFMA backward is faster there) with the lse of ign_attn_fwd_x6.  The strided form writes the three gradients into one
    (B, max(L, S), 3, H, E) buffer; what it does not own stays untouched."""
    dev = _dev()
    _lib, _ = _mod()
    lib, E = _lib.lib(), 128
    B, H = C.batch_heads(E)
    scale = C.scale_of(E)
    q, k, v, go = (t.to(dev) for t in C.edge_inputs(L, S, E))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    out = torch.empty(B, L, H, E, device=dev)
    lse = torch.empty(B, H, L, device=dev)
    delta = torch.empty(B, H, L, device=dev)
    strides = (L * H * E, H * E, S * H * E, H * E, S * H * E, H * E)
    _lib.check(lib.ign_attn_fwd_x6(ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse), B, L, S, H, E, *strides, scale, _lib.stream()),
               "ign_attn_fwd_x6")
    N = max(L, S)
    if strided:
        buf = torch.full((B, N, 3, H, E), float("nan"), device=dev)
        gq, gk, gv = buf[:, :L, 0], buf[:, :S, 1], buf[:, :S, 2]
        name, tail = "ign_attn_bwd_x6_strided", (buf.stride(0), buf.stride(1), 0)
    else:
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        name, tail = "ign_attn_bwd_x6", ()
    _lib.check(getattr(lib, name)(ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse), ptr(go), ptr(gq), ptr(gk), ptr(gv), ptr(delta), B, L,
                                  S, H, E, *strides, scale, _lib.stream(), *tail), name)
    torch.cuda.synchronize()
    ref = C.edge_reference(L, S, E)
    c = _Case("unrouted", f"{name} L={L} S={S}")
    for what, t in (("out", out), ("dq", gq), ("dk", gk), ("dv", gv)):
        c.hold(what, C.slice_err(t, ref[what]), C.FWD_TOL if what == "out" else C.GRAD_TOL)
    if strided:
        assert bool(torch.isnan(buf[:, L:, 0]).all()) and bool(torch.isnan(buf[:, S:, 1:]).all()), "rows past L / S were written"
    c.finish()


# ----------------------------------------------------------------------------------------------------------------- e. regimes
@pytest.mark.parametrize("name,amath,E", [pytest.param(r, a, E, id=f"{r}-{a}-E{E}") for r, a, E in C.regime_routes()])
def test_score_regimes_vs_float64(name, amath, E, monkeypatch):
    """Tolerance per case and tensor: max(project bound, 8 x the error of the float32 restatement of the same formula) -- the
    attainable accuracy grows with the score magnitude, a fixed number says nothing there.  No tolerance is above 4 x the project
    bound (tests/test_attn_edges_host.py).  The bf16 route: C.bf16_regime_tolerances, under the same ceiling against the bounds of
    tests/test_gpu_bf16_parity.py, on rows rescaled for it where the ceiling asks for that (C.BF16_RESCALED)."""
    dev = _dev()
    _, ops = _mod()
    ctx = _select(monkeypatch, ops, amath, E)
    inputs, scale = C.regime_inputs(name, E, amath == "bf16"), C.scale_of(E)
    got = _run(ops, ctx, inputs, scale, dev)
    c = _Case("regime", f"{name} {amath} E={E}")
    floors = C.regime_zero_floors(name, E)
    if amath == "bf16":
        _hold_bf16(c, got, C.regime_bf16_model(name, E), floors, {w: t for w, (t, _) in C.bf16_regime_tolerances(name, E).items()})
    else:
        ref, tols = C.regime_reference(name, E), C.regime_tolerances(name, E)
        for what in TENSORS:
            tol, e32, _ = tols[what]
            if what in floors and floors[what] == 0.0:
                tol = 0.0                                               # identically zero with a zero natural scale: exact zeros
            c.hold(what, C.slice_err(got[what], ref[what], floor=floors.get(what, 0.0)), tol, fp32_restatement=e32)
        if name == "uniform":                                           # p = 1 / S exactly: out is the mean of v
            mean = inputs[2].double().mean(1, keepdim=True).expand_as(ref["out"])
            c.hold("out vs mean of v", C.slice_err(got["out"], mean), C.FWD_TOL)
        _hold_inference_forward(c, ops, ctx, amath, E, inputs, scale, dev, ref["out"], tols["out"][0])
    c.finish()


# ----------------------------------------------------------------------------------------------------------------- f. views
_VB, _VL, _VS, _VH, _VE = 2, 33, 31, 3, 32


def _leaf(dev, *shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev).requires_grad_(True)


def _view_case(name, leaves, q, k, v, go):
    """q, k, v: views of `leaves` (never the leaves themselves).  The same call on contiguous, aligned copies of the views is
    the reference; the gradients are compared on the leaves, the copies' gradients pushed back through the same views."""
    _, ops = _mod()
    scale = C.scale_of(_VE)
    out = ops.attention(q, k, v, scale)
    grads = torch.autograd.grad(out, leaves, go, retain_graph=True)
    qc, kc, vc = (t.detach().clone(memory_format=torch.contiguous_format).requires_grad_(True) for t in (q, k, v))
    assert all(t.data_ptr() % 16 == 0 and t.is_contiguous() and t.stride(0) > 0 for t in (qc, kc, vc))
    out_c = ops.attention(qc, kc, vc, scale)
    grads_c = torch.autograd.grad(out_c, (qc, kc, vc), go.contiguous())
    back = torch.autograd.grad((q, k, v), leaves, grads_c)
    c = _Case("views", name)
    assert out.shape == out_c.shape == (_VB, _VL, _VH, _VE)
    c.hold("out", C.slice_err(out, out_c), C.FWD_TOL)
    for i, (g, gc, leaf) in enumerate(zip(grads, back, leaves)):
        assert g.shape == leaf.shape
        c.hold(f"grad {i}", C.whole_err(g, gc), C.GRAD_TOL)
    c.finish()


def test_batch_expanded_keys_and_values_are_copied_not_refused():
    dev = _dev()
    q0, k1, v1 = _leaf(dev, _VB, _VL, _VH, _VE, seed=1), _leaf(dev, 1, _VS, _VH, _VE, seed=2), _leaf(dev, 1, _VS, _VH, _VE, seed=3)
    k, v = k1.expand(_VB, -1, -1, -1), v1.expand(_VB, -1, -1, -1)
    assert k.stride(0) == 0 and v.stride(0) == 0
    _view_case("batch-expanded k, v", (q0, k1, v1), q0.view_as(q0), k, v, _leaf(dev, _VB, _VL, _VH, _VE, seed=4).detach())


def test_operand_four_bytes_off_alignment_is_copied():
    dev = _dev()
    buf = _leaf(dev, _VB * _VL * _VH * _VE + 1, seed=5)
    q = buf[1:].view(_VB, _VL, _VH, _VE)
    assert q.data_ptr() % 16 == 4 and q.is_contiguous()
    k0, v0 = _leaf(dev, _VB, _VS, _VH, _VE, seed=6), _leaf(dev, _VB, _VS, _VH, _VE, seed=7)
    _view_case("q 4 bytes off 16-byte alignment", (buf, k0, v0), q, k0.view_as(k0), v0.view_as(v0),
               _leaf(dev, _VB, _VL, _VH, _VE, seed=8).detach())


def test_operands_permuted_from_head_major_are_copied():
    dev = _dev()
    qh, kh, vh = (_leaf(dev, _VB, _VH, n, _VE, seed=9 + i) for i, n in enumerate((_VL, _VS, _VS)))
    q, k, v = (t.permute(0, 2, 1, 3) for t in (qh, kh, vh))
    assert q.stride(2) != _VE
    _view_case("(B, H, L, E) permuted to (B, L, H, E)", (qh, kh, vh), q, k, v, _leaf(dev, _VB, _VL, _VH, _VE, seed=12).detach())


def test_non_contiguous_output_gradient():
    dev = _dev()
    q0, k0, v0 = (_leaf(dev, _VB, n, _VH, _VE, seed=13 + i) for i, n in enumerate((_VL, _VS, _VS)))
    go = _leaf(dev, _VB, _VL, _VH, 2 * _VE, seed=16).detach()[..., ::2]
    assert not go.is_contiguous()
    _view_case("non-contiguous dO", (q0, k0, v0), q0.view_as(q0), k0.view_as(k0), v0.view_as(v0), go)
