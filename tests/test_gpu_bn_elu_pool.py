"""ops.bn_elu_pool on an MI355X at every row of tests/bn_elu_pool_cases.py, against float64 (tests/test_bn_elu_pool_host.py proves
what the table covers and what the tolerances can see).

Direct: the six entry points of csrc/ign_eegcnn_fused.hip one by one through the C ABI, each on the inputs the stage before it hands
on, each against float64 of those inputs.  Every buffer is a view inside an arena whose other words are a NaN with a payload of its
own: the words around every view and the inputs must be bitwise intact, every output word written, every element within its bound
(0 = equal: the exact regime), and a second call must repeat the first bit for bit.
End to end: ops.bn_elu_pool in training and eval mode, with and without alpha / cshift, momentum=None over two calls,
track_running_stats=False, affine=False; dalpha is held to the bound of its own S2 with no floor.
Model: one EEG-CNN training step on the BatchNorm-1 "fold" route with the input at 1e-3 of unit variance, with the gradients of
block1_bn1.weight / .bias (which reach them through dalpha alone) compared instead of skipped.
Every figure is printed and recorded before anything is asserted; IGN_BN_ELU_POOL_OUT=<file> writes the record as JSON
(tests/diag_bn_elu_pool.py -> profiles/bn_elu_pool_edges.json)."""
import copy
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import bn_elu_pool_cases as K

pytestmark = pytest.mark.gpu

GUARD = 256                       # 32-bit words in front of and behind every view
SENT = 0x7FC5A5A5                 # a quiet NaN no kernel produces (as a double made of two of them: a NaN as well)
_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("IGN_BN_ELU_POOL_OUT")
    if not _RECORD or not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(_RECORD, f, indent=1, sort_keys=True)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _mod():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    return _lib, _lib.lib()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Arena:
    """fp32 / fp64 views inside sentinel-filled buffers"""

    def __init__(self, dev):
        self.dev, self.bufs = dev, {}

    def _view(self, name, shape, dtype, kind):
        words = math.prod(shape) * (2 if dtype == torch.float64 else 1)
        buf = torch.full((2 * GUARD + words,), SENT, dtype=torch.int32, device=self.dev)
        v = buf[GUARD:GUARD + words].view(dtype).view(*shape)
        assert v.data_ptr() % 16 == 0
        self.bufs[name] = dict(buf=buf, words=words, kind=kind, was=None, view=v)
        return v

    def out(self, name, *shape, dtype=torch.float32):
        return self._view(name, shape, dtype, "out")

    def inp(self, name, x, kind="in"):
        if x is None:
            return None
        x = np.ascontiguousarray(x)
        t = torch.from_numpy(x)
        v = self._view(name, tuple(t.shape), t.dtype, kind)
        v.copy_(t)
        if kind == "in":
            self.bufs[name]["was"] = self.words(name).clone()
        return v

    def state(self, name, x):
        """read and written by the call (running statistics): the caller re-initialises it"""
        return self.inp(name, x, kind="state")

    def words(self, name):
        b = self.bufs[name]
        return b["buf"][GUARD:GUARD + b["words"]]

    def reset_outputs(self):
        for b in self.bufs.values():
            if b["kind"] == "out":
                b["buf"][GUARD:GUARD + b["words"]] = SENT

    def broken(self):
        bad = [n for n, b in self.bufs.items()
               if not (bool((b["buf"][:GUARD] == SENT).all()) and bool((b["buf"][GUARD + b["words"]:] == SENT).all()))]
        return bad + [n + " (input overwritten)" for n, b in self.bufs.items() if b["was"] is not None and not torch.equal(self.words(n), b["was"])]

    def unwritten(self, name):
        return int((self.words(name) == SENT).sum())

    def f64(self, name):
        return self.bufs[name]["view"].double().cpu().numpy()

    def snapshot(self):
        return {n: self.words(n).clone() for n, b in self.bufs.items() if b["kind"] != "in"}


class _Holds:
    """The comparisons of one row: each is printed and recorded before anything is asserted."""

    def __init__(self, table, name, route):
        self.name, self.bad = f"{table} {name}", []
        self.rec = _RECORD.setdefault(table, {}).setdefault(name, dict(route=route, outputs={}))

    def hold(self, what, got, r, **extra):
        q = K.ratio(got, r)
        err = float(np.nanmax(np.abs(np.asarray(got, np.float64).reshape(r.ref.shape) - r.ref))) if r.ref.size else 0.0
        rec = dict(ratio=q, max_abs_err=err, exact=bool(not (r.tol > 0).any()), **extra)
        self.rec["outputs"][what] = rec
        print(f"{self.name}: {what} {rec}")
        if not q <= 1.0:
            self.bad.append((what, rec))

    def equal(self, what, ok):
        self.rec["outputs"][what] = dict(ratio=0.0 if ok else float("inf"), exact=True)
        print(f"{self.name}: {what} {'ok' if ok else 'DIFFERS'}")
        if not ok:
            self.bad.append((what, "differs"))

    def finish(self):
        assert not self.bad, f"{self.name}: {self.bad}"


# ====================================================================================================================== direct ABI
def _direct_calls(c, A, L, st):
    """the six entry points in the op's order, each on the inputs direct(c) gives it; -> output name -> (entry, key)"""
    d = K.inputs(c)
    give, _ = K.direct(c)
    B, C, T, P, n = c.B, c.C, c.T, c.P, c.B * c.T
    Tp = T // P
    nws = L.ign_chan_stats_workspace_bytes(B, C) // 8
    assert nws == K.stat_slices(B) * C * 2
    v, dout = A.inp("v", d["v"]), A.inp("dout", d["dout"])
    alpha, cshift, gamma, beta = (A.inp(k, d[k]) for k in ("alpha", "cshift", "gamma", "beta"))
    sums_in, bsums_in, fold_in = A.inp("sums_in", give["sums"]), A.inp("bsums_in", give["bsums"]), A.inp("fold_in", give["fold"])
    scale, shift, mean = A.inp("scale_in", give["scale"]), A.inp("shift_in", give["shift"]), A.inp("mean_in", give["mean"])
    ka, kb, kc = (A.inp(k + "_in", give[k]) for k in ("ka", "kb", "kc"))
    rm, rv = A.state("run_mean", d["run_mean"]), A.state("run_var", d["run_var"])
    o = dict(sums=A.out("sums", C, 2, dtype=torch.float64), ws=A.out("ws", nws, dtype=torch.float64),
             scale=A.out("scale", C), shift=A.out("shift", C), fold=A.out("fold", C, 2, dtype=torch.float64),
             out=A.out("out", B, C, Tp), bsums=A.out("bsums", C, 2, dtype=torch.float64), bws=A.out("bws", nws, dtype=torch.float64),
             ka=A.out("ka", C), kb=A.out("kb", C), kc=A.out("kc", C), dgamma=A.out("dgamma", C), dbeta=A.out("dbeta", C),
             dalpha=A.out("dalpha", C) if c.affine else None, dv=A.out("dv", B, C, T))
    rm0, rv0 = torch.from_numpy(d["run_mean"]).to(A.dev), torch.from_numpy(d["run_var"]).to(A.dev)

    def prepare():
        rm.copy_(rm0)
        rv.copy_(rv0)

    def go():
        return [
            ("ign_chan_stats", L.ign_chan_stats(_p(v), _p(o["sums"]), _p(o["ws"]), B, C, T, st)),
            ("ign_bn_fold_fwd", L.ign_bn_fold_fwd(_p(sums_in), _p(alpha), _p(cshift), _p(gamma), _p(beta), _p(o["scale"]), _p(o["shift"]),
                                                  _p(o["fold"]), _p(rm), _p(rv), C, n, d["eps"], d["momentum"], st)),
            ("ign_affine_elu_pool_fwd", L.ign_affine_elu_pool_fwd(_p(v), _p(scale), _p(shift), _p(o["out"]), B, C, T, P, st)),
            ("ign_bn_elu_pool_bwd_sums", L.ign_bn_elu_pool_bwd_sums(_p(v), _p(dout), _p(scale), _p(shift), _p(mean), _p(o["bsums"]),
                                                                    _p(o["bws"]), B, C, T, P, st)),
            ("ign_bn_fold_bwd", L.ign_bn_fold_bwd(_p(bsums_in), _p(fold_in), _p(alpha), _p(gamma), _p(o["ka"]), _p(o["kb"]), _p(o["kc"]),
                                                  _p(o["dgamma"]), _p(o["dbeta"]), _p(o["dalpha"]), C, n, d["eps"], st)),
            ("ign_bn_elu_pool_bwd_apply", L.ign_bn_elu_pool_bwd_apply(_p(v), _p(dout), _p(scale), _p(shift), _p(ka), _p(kb), _p(kc),
                                                                      _p(o["dv"]), B, C, T, P, st)),
        ]
    return prepare, go


def _direct_outputs(A, c):
    s, f, b = A.f64("sums"), A.f64("fold"), A.f64("bsums")
    got = {"ign_chan_stats": dict(s=s[:, 0], q=s[:, 1]),
           "ign_bn_fold_fwd": dict(scale=A.f64("scale"), shift=A.f64("shift"), mean=f[:, 0], r=f[:, 1], run_mean=A.f64("run_mean"),
                                   run_var=A.f64("run_var")),
           "ign_affine_elu_pool_fwd": dict(out=A.f64("out")),
           "ign_bn_elu_pool_bwd_sums": dict(S1=b[:, 0], S2=b[:, 1]),
           "ign_bn_fold_bwd": {k: A.f64(k) for k in K.FOLD_BWD_OUT if k != "dalpha" or c.affine},
           "ign_bn_elu_pool_bwd_apply": dict(dv=A.f64("dv"))}
    return got


@pytest.mark.parametrize("c", K.cases(), ids=lambda c: c.id)
def test_entry_points_vs_float64(c):
    dev = _dev()
    _lib, L = _mod()
    _, refs = K.direct(c)
    A = Arena(dev)
    prepare, go = _direct_calls(c, A, L, _lib.stream())
    h = _Holds("direct", c.id, K.plan(c)["route"])
    snaps = []
    for _ in range(2):
        A.reset_outputs()
        prepare()
        rcs = go()
        torch.cuda.synchronize()
        assert all(rc == 0 for _, rc in rcs), (rcs, L.ign_last_error())
        assert A.broken() == [], "written outside a view, or an input changed"
        snaps.append(A.snapshot())
    for name, b in A.bufs.items():
        if b["kind"] == "out":
            # a double is made of two words: a written double never has the sentinel in either half
            assert A.unwritten(name) == 0, f"{name}: {A.unwritten(name)} words never written"
    A_first = {n: w for n, w in snaps[0].items()}
    # compare the FIRST call (the arena now holds the second: it must be the same bits anyway)
    for name in A_first:
        h.equal(f"{name} repeats", torch.equal(A_first[name], snaps[1][name]))
    got = _direct_outputs(A, c)
    for entry, outs in refs.items():
        for k, r in outs.items():
            h.hold(f"{entry}:{k}", got[entry][k], r)
    h.finish()


REFUSED_ENTRIES = ("ign_affine_elu_pool_fwd", "ign_bn_elu_pool_bwd_sums", "ign_bn_elu_pool_bwd_apply")


@pytest.mark.parametrize("row", K.REFUSALS, ids=[r["why"] for r in K.REFUSALS])
def test_bad_pool_width_is_refused_before_any_launch(row):
    dev = _dev()
    _lib, L = _mod()
    st = _lib.stream()
    B, C, T, P = row["B"], row["C"], row["T"], row["P"]
    assert K.bn_refuses(B, C, T, P)
    A = Arena(dev)
    g = np.random.default_rng(1)
    v, dout = A.inp("v", g.standard_normal((B, C, T)).astype(np.float32)), A.inp("dout", g.standard_normal((B, C, T)).astype(np.float32))
    cf = [A.inp(f"c{i}", g.standard_normal(C).astype(np.float32)) for i in range(6)]
    out, dv = A.out("out", B, C, T), A.out("dv", B, C, T)
    sums, ws = A.out("sums", C, 2, dtype=torch.float64), A.out("ws", L.ign_chan_stats_workspace_bytes(B, C) // 8, dtype=torch.float64)
    rcs = dict(
        ign_affine_elu_pool_fwd=L.ign_affine_elu_pool_fwd(_p(v), _p(cf[0]), _p(cf[1]), _p(out), B, C, T, P, st),
        ign_bn_elu_pool_bwd_sums=L.ign_bn_elu_pool_bwd_sums(_p(v), _p(dout), _p(cf[0]), _p(cf[1]), _p(cf[2]), _p(sums), _p(ws), B, C, T, P, st),
        ign_bn_elu_pool_bwd_apply=L.ign_bn_elu_pool_bwd_apply(_p(v), _p(dout), _p(cf[0]), _p(cf[1]), _p(cf[3]), _p(cf[4]), _p(cf[5]), _p(dv),
                                                              B, C, T, P, st))
    torch.cuda.synchronize()
    assert set(rcs) == set(REFUSED_ENTRIES)
    assert all(rc == K.IGN_E_ARG for rc in rcs.values()), rcs
    assert b"bad dimension" in L.ign_last_error()
    assert A.broken() == []
    for name in ("out", "dv", "sums", "ws"):
        assert A.unwritten(name) == A.bufs[name]["words"], f"{name} touched by a refused call"
    _RECORD.setdefault("refusals", {})[row["why"]] = dict(rc=K.IGN_E_ARG, entries=sorted(rcs))


# ====================================================================================================================== ops.bn_elu_pool
def _bn(c, dev, momentum="row", **kw):
    d = K.inputs(c)
    bn = torch.nn.BatchNorm2d(c.C, eps=d["eps"], momentum=d["momentum"] if momentum == "row" else momentum, **kw)
    with torch.no_grad():
        if bn.weight is not None:
            bn.weight.copy_(torch.from_numpy(d["gamma"]))
            bn.bias.copy_(torch.from_numpy(d["beta"]))
        if bn.running_mean is not None:
            bn.running_mean.copy_(torch.from_numpy(d["run_mean"]))
            bn.running_var.copy_(torch.from_numpy(d["run_var"]))
    return bn.to(dev)


def _op_once(c, bn, dev, calls=1):
    """`calls` forward passes (the running statistics move each time), backward through the last -> name -> tensor"""
    from ign_hip import ops
    d = K.inputs(c)
    v = torch.from_numpy(d["v"]).to(dev).requires_grad_(True)
    a = torch.from_numpy(d["alpha"]).to(dev).requires_grad_(True) if c.affine else None
    cs = torch.from_numpy(d["cshift"]).to(dev).requires_grad_(True) if c.affine else None
    for p in bn.parameters():
        p.grad = None
    for _ in range(calls):
        out = ops.bn_elu_pool(v, bn, c.P, alpha=a, cshift=cs)
    (out * torch.from_numpy(d["dout"]).to(dev)).sum().backward()
    torch.cuda.synchronize()
    got = dict(out=out.detach(), dv=v.grad)
    if bn.weight is not None:
        got.update(dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    if c.affine:
        got.update(dalpha=a.grad, dc=cs.grad)
    if bn.running_mean is not None:
        got.update(run_mean=bn.running_mean.detach().clone(), run_var=bn.running_var.detach().clone())
    return got


def _hold_op(h, got, R, tag="", keys=K.OP_OUTPUTS):
    for k in keys:
        if k in R and k in got and got[k] is not None:
            h.hold(tag + k, got[k].double().cpu().numpy(), R[k])


def _repeats(h, one, two, tag=""):
    for k in one:
        same = (one[k] is None and two[k] is None) or (one[k] is not None and two[k] is not None and torch.equal(one[k], two[k]))
        h.equal(f"{tag}{k} repeats", same)


@pytest.mark.parametrize("c", K.op_cases(), ids=lambda c: c.id)
def test_op_training_vs_float64(c):
    """out, dv, dgamma, dbeta, dalpha and the running statistics; dalpha at the bound of its own S2, no floor; dc exactly 0"""
    dev = _dev()
    _mod()
    R = K.reference_op(c)
    h = _Holds("op_train", c.id, K.plan(c)["route"])
    runs = [_op_once(c, _bn(c, dev).train(), dev) for _ in range(2)]
    _hold_op(h, runs[0], R)
    assert ("dalpha" in runs[0]) == c.affine == ("dalpha" in R)
    if c.affine:
        dc = runs[0]["dc"]
        h.equal("dc is exactly zero", dc is None or float(dc.abs().max()) == 0.0)
        da, dg = np.abs(R["dalpha"].ref).max(), np.abs(R["dgamma"].ref).max()
        h.rec["dalpha_over_dgamma"] = float(da / dg) if dg > 0 else None
        h.rec["dalpha_tol_over_dalpha"] = float(R["dalpha"].tol.max() / da) if da > 0 else None
    if c.regime.startswith("offset"):           # the DC sensitivity on record: errors in units of sigma (= 1 here) against |mean| / sigma
        d = K.inputs(c)
        sig = float(d["v"].astype(np.float64).std(axis=(0, 2)).mean())
        h.rec["dc_sensitivity"] = dict(
            mean_over_sigma=float(c.regime[6:]),
            out_err_over_sigma=float(np.abs(runs[0]["out"].double().cpu().numpy() - R["out"].ref).max() / sig),
            dv_err_over_max_dv=float(np.abs(runs[0]["dv"].double().cpu().numpy() - R["dv"].ref).max() / np.abs(R["dv"].ref).max()))
    _repeats(h, runs[0], runs[1])
    h.finish()


EVAL_CASES = [c for c in K.op_cases() if c.regime in ("gauss", "offset16", "epsdom_eps")]


@pytest.mark.parametrize("c", EVAL_CASES, ids=lambda c: c.id)
def test_op_eval_vs_float64(c):
    """eval mode: the running statistics as an affine map in front of the apply kernels; they do not move"""
    dev = _dev()
    _mod()
    R = K.reference_eval(c)
    d = K.inputs(c)
    h = _Holds("op_eval", c.id, K.plan(c)["route"])
    runs = [_op_once(c, _bn(c, dev).eval(), dev) for _ in range(2)]
    _hold_op(h, runs[0], R, keys=("out", "dv", "dgamma", "dbeta", "dalpha", "dc"))
    h.equal("running statistics untouched", bool(np.array_equal(runs[0]["run_mean"].cpu().numpy(), d["run_mean"])
                                                 and np.array_equal(runs[0]["run_var"].cpu().numpy(), d["run_var"])))
    _repeats(h, runs[0], runs[1])
    h.finish()


@pytest.mark.parametrize("name,kw,training", K.HOST_BRANCHES, ids=[b[0] for b in K.HOST_BRANCHES])
@pytest.mark.parametrize("affine", [True, False], ids=["alpha", "noalpha"])
def test_op_host_branches_vs_float64(name, kw, training, affine):
    """momentum=None (cumulative average over two calls), track_running_stats=False (batch statistics in eval too, nothing to
    update), affine=False (no weight / bias)"""
    dev = _dev()
    _mod()
    c = K.Case("gauss", *K.HOST_SHAPE, affine=affine, bn_affine=kw.get("affine", True))
    d = K.inputs(c)
    h = _Holds("op_host_branches", f"{name}-{c.name}", K.plan(c)["route"])
    calls = 2 if "momentum" in kw else 1
    tracked = kw.get("track_running_stats", True)
    batch_stats = training or not tracked
    R = K.reference_op(c, momentum="cumulative" if "momentum" in kw else None, calls=calls) if batch_stats else K.reference_eval(c)
    runs = []
    for _ in range(2):
        bn = _bn(c, dev, **({"momentum": None} if "momentum" in kw else {}), **{k: v for k, v in kw.items() if k != "momentum"})
        bn.train(training)
        runs.append(_op_once(c, bn, dev, calls=calls))
        if tracked:
            assert int(bn.num_batches_tracked) == (calls if training else 0)
        else:
            assert bn.running_mean is None and bn.num_batches_tracked is None
    keys = ("out", "dv", "dalpha") + (("dgamma", "dbeta") if kw.get("affine", True) else ()) + (("run_mean", "run_var") if training else ())
    _hold_op(h, runs[0], R, keys=keys + (() if batch_stats else ("dc",)))
    if not training and tracked:
        h.equal("running statistics untouched", bool(np.array_equal(runs[0]["run_mean"].cpu().numpy(), d["run_mean"])))
    if not kw.get("affine", True):
        assert "dgamma" not in runs[0]
    _repeats(h, runs[0], runs[1])
    h.finish()


# ====================================================================================================================== the model row
def test_eegcnn_step_on_millivolt_input_compares_block1_bn1():
    """One EEG-CNN training step on the BatchNorm-1 `fold` route with the input at 1e-3 of unit variance: BatchNorm-1 is then
    eps-dominated (its batch variance is below eps) and alpha stays ~ gamma / sqrt(eps) on tiny data.  dalpha is the only path of a
    gradient to block1_bn1.weight through BatchNorm-2 (in float64 that gradient is 2.7e-4 of the largest here, 14x its share at unit
    scale); block1_bn1.bias only moves c, whose gradient is exactly 0.  Both are COMPARED with float64 instead of skipped: their bound
    is 4x the error of the same layer sequence in plain fp32 torch on the same inputs (the fused path reorders the same roundings),
    which for the weight is ~1e-3 of the gradient itself; every other parameter keeps MODEL_TOL of its scale."""
    dev = _dev()
    _mod()
    import eegcnn_route_cases as Rt
    from test_gpu_baselines import _eegcnn_reference_ops
    from test_gpu_eegcnn_routes import _model
    shape = K.MODEL_ROW["shape"]
    B, C, T, k1 = shape[:4]
    assert Rt.bn1_route(T, k1, shape[5]) == "fold" and any(r[1] == shape for r in Rt.MODEL_CASES)
    m = _model(shape, dev)
    ref64, ref32 = copy.deepcopy(m).double().train(), copy.deepcopy(m).float().train()
    m.to(dev).train()
    g = torch.Generator().manual_seed(B + T)
    x = (torch.randn(B, C, T, generator=g) * 1.5 + 0.2) * K.MODEL_ROW["input_scale"]
    a = m(x.to(dev))
    b64 = _eegcnn_reference_ops(ref64, x.double())
    b32 = _eegcnn_reference_ops(ref32, x)
    names = [n for n, _ in m.named_parameters()]
    ga = torch.autograd.grad(a.square().sum(), list(m.parameters()), allow_unused=True)
    g64 = torch.autograd.grad(b64.square().sum(), list(ref64.parameters()))
    g32 = torch.autograd.grad(b32.square().sum(), list(ref32.parameters()))
    torch.cuda.synchronize()
    h = _Holds("model", "fold-millivolt", "EEGcnn " + str(shape) + ", BatchNorm-1 route fold, input x 1e-3")
    top = float(max(t.abs().max() for t in g64))
    scale_tol = lambda ref: K.Ref(ref, Rt.MODEL_TOL * max(float(np.abs(ref).max()), 1e-30))
    h.hold("out", a.detach().double().cpu().numpy(), scale_tol(b64.detach().numpy()))
    for n, u, v64, v32 in zip(names, ga, g64, g32):
        ref = v64.numpy()
        if n in Rt.ZERO_GRAD_PARAMS:
            u = torch.zeros_like(v32) if u is None else u            # no path at all: an exact zero
            e32 = float((v32.double() - v64).abs().max())
            assert e32 > 0
            h.hold("grad." + n, u.double().cpu().numpy(), K.Ref(ref, K.MODEL_ROW["fp32_factor"] * e32),
                   fp32_torch_error=e32, over_largest_gradient=float(np.abs(ref).max() / top), largest=float(np.abs(ref).max()))
        else:
            assert u is not None and torch.isfinite(u).all(), n
            h.hold("grad." + n, u.double().cpu().numpy(), scale_tol(ref))
    h.finish()
