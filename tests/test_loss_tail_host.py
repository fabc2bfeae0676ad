"""Loss tail, host side: what ops.ign_loss, ops.ign_crps_loss, ops.crps_loss and ops.gini_gate hand to the C ABI -- which entry
point, every argument at the position include/ign_abi.h gives its NAME, which buffers are allocated and how they alias -- what
their backward passes return (the saved gradients themselves under the unit root of ops.backward, one value per forward input),
every error text, and the structure rule (the two gated entry points are named in the one launcher only).  Needs neither a device
nor libign_hip.so: the public functions run on CPU tensors against a stand-in library that records the call.  Everything but the
expert-shape check of ops.ign_loss and the structure rule was first run against the two hand-written nodes this layout replaced,
so the traces pin that behaviour, not this code's."""
import ast
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM = 0x5EED
B, N, BETA = 5, 7, 0.75
GATED = {"ign_loss": "ign_loss_fwd_bwd_reg", "ign_crps_loss": "ign_loss_crps_fwd_bwd_reg"}


def _mods():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops, _lib
    return ops, _lib


# ---------------------------------------------------------------- stand-in library
class _StandIn:
    """Every attribute is an entry point that records (name, args) and answers 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture
def host(monkeypatch):
    """-> (ops, _lib, rec, labels, seen): the recorded calls, the labels given to _lib.check, and every tensor whose address went
    to the library, by address (kept alive, so no address is handed out twice within a test)."""
    ops, _lib = _mods()
    rec, labels, seen = _StandIn(), [], {}
    real_ptr = ops._ptr

    def ptr(t):
        if t is not None:
            seen[t.data_ptr()] = t
        return real_ptr(t)
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "check", lambda rc, what: labels.append(what))
    monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(STREAM))
    monkeypatch.setattr(ops, "_need_gpu", lambda name, *ts: None)
    monkeypatch.setattr(ops, "_ptr", ptr)
    return ops, _lib, rec, labels, seen


def _header_params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
    assert m, name
    return [re.split(r"[\s*]+", p.strip())[-1] for p in m.group(1).split(",")]


def _named(_lib, call, name):
    """The recorded call as {header parameter name: address (None = null) or number}: the entry point is `name`, it is declared in
    _lib.SIGNATURES, and the argument count is the signature's and the header's."""
    got, args = call
    assert got == name
    params = _header_params(name)
    assert name in _lib.SIGNATURES and len(args) == len(_lib.SIGNATURES[name][1]) == len(params), name
    return dict(zip(params, [a.value if isinstance(a, ctypes.c_void_p) else a for a in args]))


def _experts(dtype=torch.float32, grad=True):
    gen = torch.Generator().manual_seed(3)
    s, d = torch.randn(B, N, generator=gen).to(dtype), torch.randn(B, N, generator=gen).to(dtype)
    return s.requires_grad_(grad), d.requires_grad_(grad)


def _criterion(op):
    """The criterion arguments between `dnn` and `beta` / `reg`: labels, or (target (B, 1), edges)."""
    if op == "ign_loss":
        return (torch.arange(B) % N,)
    edges = torch.cat([torch.linspace(-1.0, 1.0, N - 1, dtype=torch.float64), torch.tensor([float("inf")], dtype=torch.float64)])
    return torch.linspace(-2.0, 2.0, B).reshape(B, 1), edges


class _Ctx:
    """What forward / backward of an autograd.Function ask of their ctx."""

    def mark_non_differentiable(self, *ts):
        self.non_differentiable = ts

    def set_materialize_grads(self, flag):
        self.materialize = flag

    def save_for_backward(self, *ts):
        self.saved_tensors = ts


# ---------------------------------------------------------------- the gated tails: forward
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_reg", [False, True])
@pytest.mark.parametrize("op", sorted(GATED))
def test_gated_tail_forward_trace(host, op, with_reg, dtype):
    ops, _lib, rec, labels, seen = host
    s, d = _experts(dtype)
    crit = _criterion(op)
    reg = torch.full((1,), 0.25, requires_grad=True) if with_reg else None
    loss, out, eta = getattr(ops, op)(s, d, *crit, BETA, reg=reg)
    (call,) = rec.calls
    assert labels == [GATED[op]]
    got = _named(_lib, call, GATED[op])
    assert (got["B"], got["N"], got["beta"], got["stream"]) == (B, N, BETA, STREAM)
    for k in ("sbm", "dnn"):                                   # the experts arrive as dense fp32 (B, N), whatever they were
        t = seen[got[k]]
        assert t.dtype == torch.float32 and t.shape == (B, N) and t.is_contiguous()
    if dtype == torch.float32:
        assert got["sbm"] == s.data_ptr() and got["dnn"] == d.data_ptr()
    assert got["reg"] == (reg.data_ptr() if with_reg else None)
    assert got["gdnn"] - got["gsbm"] == 4 * B * N              # one (2, B, N) buffer
    assert seen[got["gsbm"]].dtype == torch.float32
    lossbuf = got["loss2" if op == "ign_loss" else "loss3"]
    assert loss.data_ptr() == lossbuf + 8 and loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    assert out.data_ptr() == got["out"] and out.shape == (B, N) and out.dtype == torch.float32 and not out.requires_grad
    assert eta.data_ptr() == got["eta"] and eta.shape == (B, 1) and eta.dtype == torch.float32 and not eta.requires_grad
    if op == "ign_loss":
        y = seen[got["labels"]]
        assert y.dtype == torch.int64 and got["labels"] == crit[0].data_ptr()
    else:
        target, edges = seen[got["target"]], seen[got["edges"]]
        assert target.dtype == torch.float32 and target.shape == (B,) and got["target"] == crit[0].data_ptr()
        assert edges.dtype == torch.float64 and edges.shape == (N,) and got["edges"] == crit[1].data_ptr()


def test_crps_tail_converts_target_and_edges(host):
    ops, _lib, rec, _, seen = host
    s, d = _experts()
    target, edges = _criterion("ign_crps_loss")
    ops.ign_crps_loss(s, d, target.double(), edges.float(), BETA)
    got = _named(_lib, rec.calls[0], "ign_loss_crps_fwd_bwd_reg")
    assert seen[got["target"]].dtype == torch.float32 and seen[got["edges"]].dtype == torch.float64
    assert seen[got["edges"]].shape == (N,) and seen[got["target"]].shape == (B,)


# ---------------------------------------------------------------- the gated tails: backward
@pytest.mark.parametrize("with_reg", [False, True])
@pytest.mark.parametrize("op,node,n_in", [("ign_loss", "IgnLossFn", 5), ("ign_crps_loss", "IgnCrpsLossFn", 6)])
def test_gated_tail_backward(host, op, node, n_in, with_reg):
    ops, _lib, rec, _, _ = host
    s, d = _experts(grad=False)
    reg = torch.full((1,), 0.25) if with_reg else None
    fn, ctx = getattr(ops, node), _Ctx()
    loss, out, eta = fn.forward(ctx, s, d, *_criterion(op), BETA, reg)
    got = _named(_lib, rec.calls[0], GATED[op])
    assert {t.data_ptr() for t in ctx.non_differentiable} == {out.data_ptr(), eta.data_ptr()} and ctx.materialize is False
    del rec.calls[:]
    unit = ops.unit_grad(loss.device)
    grads = fn.backward(ctx, unit, None, None)                 # the root of ops.backward(): the saved halves, no multiply
    assert isinstance(grads, tuple) and len(grads) == n_in
    assert grads[0].data_ptr() == got["gsbm"] and grads[1].data_ptr() == got["gdnn"]
    assert grads[0].shape == grads[1].shape == (B, N)
    assert all(g is None for g in grads[2:-1])
    assert (grads[-1].shape == reg.shape and grads[-1].data_ptr() == unit.data_ptr()) if with_reg else grads[-1] is None
    two = torch.tensor(2.0)
    scaled = fn.backward(ctx, two, None, None)                 # any other root: new tensors
    assert len(scaled) == n_in and scaled[0].shape == scaled[1].shape == (B, N)
    assert not {scaled[0].data_ptr(), scaled[1].data_ptr()} & {got["gsbm"], got["gdnn"]}
    assert (scaled[-1].shape == reg.shape) if with_reg else scaled[-1] is None
    nothing = fn.backward(ctx, None, None, None)
    assert isinstance(nothing, tuple) and len(nothing) == n_in and all(g is None for g in nothing)
    assert not rec.calls                                       # the backward launches nothing


def test_ops_backward_on_a_cpu_loss_is_plain_backward(host):
    ops = host[0]
    w = torch.ones(3, requires_grad=True)
    ops.backward((w * 2).sum())
    assert torch.equal(w.grad, torch.full((3,), 2.0))


# ---------------------------------------------------------------- crps_loss
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_crps_loss_trace(host, dtype):
    ops, _lib, rec, labels, seen = host
    z = _experts(dtype)[0]
    target, edges = _criterion("ign_crps_loss")
    loss = ops.crps_loss(z, target, edges)
    (call,) = rec.calls
    assert labels == ["ign_crps_fwd_bwd"]
    got = _named(_lib, call, "ign_crps_fwd_bwd")
    assert (got["B"], got["N"], got["stream"]) == (B, N, STREAM)
    assert seen[got["logits"]].dtype == torch.float32 and (dtype != torch.float32 or got["logits"] == z.data_ptr())
    assert got["target"] == target.data_ptr() and got["edges"] == edges.data_ptr()
    assert loss.data_ptr() == got["loss_out"] and loss.dim() == 0 and loss.requires_grad
    assert seen[got["grad"]].shape == (B, N) and seen[got["grad"]].dtype == torch.float32


def test_crps_loss_backward(host):
    ops, _lib, rec, _, _ = host
    ctx = _Ctx()
    loss = ops.CrpsLossFn.forward(ctx, _experts(grad=False)[0], *_criterion("ign_crps_loss"))
    got = _named(_lib, rec.calls[0], "ign_crps_fwd_bwd")
    del rec.calls[:]
    grads = ops.CrpsLossFn.backward(ctx, ops.unit_grad(loss.device))
    assert len(grads) == 3 and grads[0].data_ptr() == got["grad"] and grads[1] is None and grads[2] is None
    scaled = ops.CrpsLossFn.backward(ctx, torch.tensor(2.0))
    assert len(scaled) == 3 and scaled[0].shape == (B, N) and scaled[0].data_ptr() != got["grad"]
    assert not rec.calls


# ---------------------------------------------------------------- gini_gate
@pytest.mark.parametrize("gating_value,gv", [(None, (0.0, 0)), (0.3, (0.3, 1))])
def test_gini_gate_forward_trace(host, gating_value, gv):
    ops, _lib, rec, labels, seen = host
    s, d = _experts(torch.bfloat16)
    out, eta = ops.gini_gate(s, d, gating_value)
    (call,) = rec.calls
    assert labels == ["ign_gate_fwd"]
    got = _named(_lib, call, "ign_gate_fwd")
    assert (got["B"], got["N"], got["gating_value"], got["use_gating_value"], got["stream"]) == (B, N, *gv, STREAM)
    assert seen[got["sbm"]].dtype == seen[got["dnn"]].dtype == torch.float32
    assert out.data_ptr() == got["out"] and out.shape == (B, N) and out.requires_grad
    assert eta.data_ptr() == got["eta"] and eta.shape == (B, 1) and eta.dtype == torch.float32


@pytest.mark.parametrize("have", ["gout", "geta", "both", "none"])
@pytest.mark.parametrize("gating_value,gv", [(None, (0.0, 0)), (0.3, (0.3, 1))])
def test_gini_gate_backward_trace(host, gating_value, gv, have):
    ops, _lib, rec, labels, seen = host
    s, d = _experts(grad=False)
    ctx = _Ctx()
    ops.GiniGateFn.forward(ctx, s, d, gating_value)
    del rec.calls[:], labels[:]
    gout = torch.ones(B, N) if have in ("gout", "both") else None
    geta = torch.ones(B, 1) if have in ("geta", "both") else None
    grads = ops.GiniGateFn.backward(ctx, gout, geta)
    assert isinstance(grads, tuple) and len(grads) == 3 and grads[2] is None
    if have == "none":
        assert grads == (None, None, None) and not rec.calls
        return
    (call,) = rec.calls
    assert labels == ["ign_gate_bwd"]
    got = _named(_lib, call, "ign_gate_bwd")
    assert (got["B"], got["N"], got["gating_value"], got["use_gating_value"], got["stream"]) == (B, N, *gv, STREAM)
    assert got["sbm"] == s.data_ptr() and got["dnn"] == d.data_ptr()
    assert got["geta"] == (geta.data_ptr() if geta is not None else None)
    if gout is not None:
        assert got["gout"] == gout.data_ptr()
    else:                                                      # only eta carries a gradient: the kernel gets zeros for gout
        assert seen[got["gout"]].shape == (B, N) and not seen[got["gout"]].any()
    assert grads[0].data_ptr() == got["gsbm"] and grads[1].data_ptr() == got["gdnn"]
    assert grads[0].shape == grads[1].shape == (B, N)


# ---------------------------------------------------------------- error texts, and their order
def _raises(_lib, text):
    return pytest.raises(_lib.IgnError, match="^" + re.escape(text) + "$")


@pytest.mark.parametrize("op", sorted(GATED))
def test_gated_tail_error_texts(host, op):
    ops, _lib, rec, _, _ = host
    fn = getattr(ops, op)
    s, d = _experts()
    crit = _criterion(op)
    wide = torch.zeros(B, 257)
    wide_crit = crit if op == "ign_loss" else (crit[0], torch.zeros(257, dtype=torch.float64))
    with _raises(_lib, f"{op}: the regulariser must be one value, got (2,)"):
        fn(s, d, *crit, BETA, reg=torch.zeros(2))
    with _raises(_lib, f"{op}: N=257 classes > 256, the widest class head the HIP kernels take (IGN_HEAD_NMAX)"):
        fn(wide, wide, *wide_crit, BETA)
    with _raises(_lib, f"{op}: N=257 classes > 256, the widest class head the HIP kernels take (IGN_HEAD_NMAX)"):
        fn(wide, wide, *wide_crit, BETA, reg=torch.zeros(2))   # the class count is checked before the regulariser
    assert not rec.calls


@pytest.mark.parametrize("op", sorted(GATED))
def test_gated_tail_refuses_experts_of_different_shapes(host, op):
    """Before everything else: the kernel reads B*N elements of both.  (ops.ign_loss did not check this before the two tails
    shared their host path.)"""
    ops, _lib, rec, _, _ = host
    fn = getattr(ops, op)
    s, d = _experts()
    crit = _criterion(op)
    with _raises(_lib, f"{op}: expert logits ({B}, {N}) vs ({B}, {N + 1})"):
        fn(s, torch.zeros(B, N + 1), *crit, BETA, reg=torch.zeros(2))
    with _raises(_lib, f"{op}: expert logits ({B}, 257) vs ({B}, {N})"):
        fn(torch.zeros(B, 257), d, *crit, BETA)
    assert not rec.calls


@pytest.mark.parametrize("op", ["crps_loss", "ign_crps_loss"])
def test_crps_target_and_edge_counts(host, op):
    ops, _lib, rec, _, _ = host
    s, d = _experts()
    target, edges = _criterion("ign_crps_loss")
    fn = (lambda t, e, **kw: ops.crps_loss(s, t, e)) if op == "crps_loss" else (lambda t, e, **kw: ops.ign_crps_loss(s, d, t, e, BETA, **kw))
    with _raises(_lib, f"{op}: logits ({B}, {N}) need {B} targets and {N} bin edges, got {B - 1} and {N}"):
        fn(target[:-1], edges)
    with _raises(_lib, f"{op}: logits ({B}, {N}) need {B} targets and {N} bin edges, got {B} and {N + 1}"):
        fn(target, torch.cat([edges, edges[-1:]]), reg=torch.zeros(2))    # before the regulariser
    if op == "crps_loss":
        with _raises(_lib, "crps_loss: N=257 classes > 256, the widest class head the HIP kernels take (IGN_HEAD_NMAX)"):
            ops.crps_loss(torch.zeros(B, 257), target[:-1], edges)        # the class count before the target / edge counts
    assert not rec.calls


# ---------------------------------------------------------------- structure
def test_gated_entry_points_are_named_in_the_launcher_only():
    tree = ast.parse(open(os.path.join(ROOT, "speech-imagery-eeg_amd", "ign_hip", "ops.py")).read())
    names = set(GATED.values())

    def mentions(node):
        return {n.attr for n in ast.walk(node) if isinstance(n, ast.Attribute) and n.attr in names} | \
               {n.value for n in ast.walk(node) if isinstance(n, ast.Constant) and n.value in names}
    users = {fn.name: mentions(fn) for fn in ast.walk(tree) if isinstance(fn, ast.FunctionDef) and mentions(fn)}
    assert users == {"_loss_tail": names}
    outside = [n for n in tree.body if not isinstance(n, (ast.FunctionDef, ast.ClassDef)) and mentions(n)]
    assert not outside
