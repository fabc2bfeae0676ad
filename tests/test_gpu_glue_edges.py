"""The class head, the two SBM regularisers (csrc/ign_head.hip) and the FCN BatchNorm / pool / bound glue (csrc/ign_bn.hip) through the
C ABI at every edge of tests/glue_edge_cases.py, against float64 (tests/test_glue_edges_host.py proves what the table covers and what
the tolerances can see).

Every buffer a kernel touches is a view inside an arena whose every other word is a NaN with a payload of its own: outputs are
prefilled with it, inputs are surrounded by it (the inputs of the maximum kernels, which drop NaNs, by 3e38).  Each case asserts:
the words around every view and the inputs are bitwise intact; every output element that has to be written was, and no other; every
element is within its bound of float64 (0 = equal, the exact regime); a second call repeats the first bit for bit.  Every figure is
printed and recorded before anything is asserted; IGN_GLUE_EDGES_OUT=<file> writes the record as JSON (tests/diag_glue_edges.py ->
profiles/glue_edges.json)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import glue_edge_cases as G

pytestmark = pytest.mark.gpu

GUARD = 256                       # words in front of and behind every view
SENT = 0x7FC5A5A5                 # a quiet NaN no kernel produces
FENCE = 3e38                      # around the inputs of the maximum kernels: fmaxf drops a NaN, not this
_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("IGN_GLUE_EDGES_OUT")
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


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])


class Arena:
    """views inside sentinel-filled buffers"""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def _view(self, name, shape, is_out):
        n = math.prod(shape)
        buf = torch.full((2 * GUARD + n,), SENT, dtype=torch.int32, device=self.dev)
        self.bufs.append([name, buf, n, is_out, None])
        v = buf.view(torch.float32)[GUARD:GUARD + n].view(*shape)
        assert v.data_ptr() % 16 == 0
        return v

    def out(self, name, *shape):
        return self._view(name, shape, True)

    def inp(self, name, x):
        if x is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        v = self._view(name, tuple(t.shape), False)
        v.copy_(t)
        self.bufs[-1][4] = self.words(name).clone()
        return v

    def state(self, name, x):
        """read and written by the call (a bound slot, running statistics, a workspace): the caller re-initialises it"""
        if x is None:
            return None
        v = self.inp(name, x)
        self.bufs[-1][4] = None
        return v

    def fenced(self, name, x, lead=4):
        """x with `lead` floats of 3e38 in front and 4 behind, -> the view of x alone (lead = 5: one float off 16-byte alignment)"""
        full = np.full(lead + x.size + 4, FENCE, np.float32)
        full[lead:lead + x.size] = x
        return self.inp(name, full)[lead:lead + x.size]

    def reset_outputs(self):
        for _, buf, n, is_out, _ in self.bufs:
            if is_out:
                buf[GUARD:GUARD + n] = SENT

    def broken_guards(self):
        """the views whose surroundings changed, and the inputs that did (bitwise)"""
        bad = [name for name, buf, n, _, _ in self.bufs
               if not (bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all()))]
        return bad + [name + " (input overwritten)" for name, buf, n, _, was in self.bufs
                      if was is not None and not torch.equal(buf[GUARD:GUARD + n], was)]

    def words(self, name):
        buf, n = next((b, n) for nm, b, n, _, _ in self.bufs if nm == name)
        return buf[GUARD:GUARD + n]

    def f64(self, name, shape=None):
        v = self.words(name).view(torch.float32).double().cpu().numpy()
        return v if shape is None else v.reshape(shape)

    def outputs(self):
        return {name: buf[GUARD:GUARD + n].clone() for name, buf, n, is_out, _ in self.bufs if is_out}


class _Holds:
    """The comparisons of one case: each is printed and recorded before anything is asserted."""

    def __init__(self, c, route=None):
        self.name, self.bad = c.id, []
        route = G.plan(c).get("route", "") if route is None else route
        self.rec = _RECORD.setdefault(c.entry, {}).setdefault(f"{c.name} {c.regime}", dict(route=route, outputs={}))

    def hold(self, what, got, r):
        got = np.asarray(got, np.float64).reshape(r.ref.shape)
        diff = np.abs(got - r.ref)
        diff = np.where(np.isnan(diff), np.inf, diff)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(r.tol > 0, diff / np.where(r.tol > 0, r.tol, 1.0), np.where(diff == 0, 0.0, np.inf))
        ratio = float(q.max()) if q.size else 0.0
        rec = dict(ratio=ratio, d=r.d, chain=r.chain, exact=bool(not (r.tol > 0).any()), max_abs_err=float(diff.max()) if q.size else 0.0)
        self.rec["outputs"][what] = rec
        print(f"{self.name}: {what} {rec}")
        if not ratio <= 1.0:
            self.bad.append((what, rec))

    def equal(self, what, ok):
        self.rec["outputs"][what] = dict(ratio=0.0 if ok else float("inf"), exact=True, d=0, chain=0)
        print(f"{self.name}: {what} {'ok' if ok else 'DIFFERS'}")
        if not ok:
            self.bad.append((what, "differs"))

    def finish(self):
        assert not self.bad, f"{self.name}: {self.bad}"


def _run(c, A, go, refs, unwritten=None, prepare=None, late=None):
    """go() -> return code.  refs: output -> Ref.  unwritten: output -> bool mask (numpy, flat) of the words that must stay
    sentinel (default: none).  prepare(): (re)initialises the state buffers before each call.  late(h, first): further checks on the
    first call's outputs.  Asserts the guards, full writes, the bounds and a bitwise second call."""
    _lib, L = _mod()
    h = _Holds(c)
    unwritten = unwritten or {}
    outs = []
    for _ in range(2):
        A.reset_outputs()
        if prepare:
            prepare()
        rc = go()
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.ign_last_error())
        assert A.broken_guards() == [], "written outside a view, or an input changed"
        outs.append((A.outputs(), {nm: A.words(nm).clone() for nm, _, _, is_out, was in A.bufs if not is_out and was is None}))
    first, state = outs[0]
    for name, words in first.items():
        sent = (words == SENT).cpu().numpy()
        must_stay = unwritten.get(name, np.zeros(sent.shape, bool))
        assert not (sent & ~must_stay).any(), f"{name}: {int((sent & ~must_stay).sum())} elements never written"
        assert (sent | ~must_stay).all(), f"{name}: {int((~sent & must_stay).sum())} elements written that must not be"
    for name, r in refs.items():
        src = first[name] if name in first else state[name]
        got = src.view(torch.float32).double().cpu().numpy()
        if name in unwritten:
            keep = ~unwritten[name]
            h.hold(name, got[keep], G.Ref(r.ref.reshape(-1), r.tol.reshape(-1), r.d, r.chain))
        else:
            h.hold(name, got, r)
    if late:
        late(h, {**{k: v for k, v in state.items()}, **first})
    for name in first:
        h.equal(f"{name} repeats", torch.equal(first[name], outs[1][0][name]))
    for name in state:
        h.equal(f"{name} repeats", torch.equal(state[name], outs[1][1][name]))
    h.finish()


def _f(words):
    return words.view(torch.float32).double().cpu().numpy()


def _ids(cs):
    return [pytest.param(c, id=f"{c.name}-{c.regime}") for c in cs]


# ===================================================================================================================== head
@pytest.mark.parametrize("c", _ids(G.of("head_fwd")))
def test_head_fwd(c):
    dev = _dev()
    _lib, L = _mod()
    A, d, s = Arena(dev), G.inputs(c), _lib.stream()
    X, W, bias = A.inp("X", d["X"]), A.inp("W", d["W"]), A.inp("bias", d["bias"])
    out = A.out("out", c.B, c.N)
    _run(c, A, lambda: L.ign_head_fwd(_p(X), _p(W), _p(bias), _p(out), c.B, c.F, c.N, c.F + c.pad, s), G.reference(c))


@pytest.mark.parametrize("c", _ids(G.of("head_bwd")))
def test_head_bwd(c):
    dev = _dev()
    _lib, L = _mod()
    A, d, s = Arena(dev), G.inputs(c), _lib.stream()
    ldx = c.F + c.pad
    g, X, W = A.inp("g", d["g"]), A.inp("X", d["X"]), A.inp("W", d["W"])
    add, scale = A.inp("add", d.get("add")), A.inp("scale", d.get("scale"))
    gX = A.out("gX", c.B, ldx) if "x" in c.mode else None
    gW = A.out("gW", c.N, c.F) if "w" in c.mode else None
    gb = A.out("gbias", c.N) if c.gbias else None
    unwritten = {}
    if gX is not None:
        m = np.zeros((c.B, ldx), bool)
        m[:, c.F:] = True                             # the row padding of gX is not the kernel's
        unwritten["gX"] = m.reshape(-1)
    if gb is not None and gW is None:
        unwritten["gbias"] = np.ones(c.N, bool)        # gbias rides on the weight-gradient blocks: without gW it is not touched
    if c.add == "none":
        go = lambda: L.ign_head_bwd(_p(g), _p(X), _p(W), _p(gX), _p(gW), _p(gb), c.B, c.F, c.N, ldx, s)
    else:
        go = lambda: L.ign_head_bwd_acc(_p(g), _p(X), _p(W), _p(gX), _p(gW), _p(gb), _p(add), _p(scale), c.B, c.F, c.N, ldx, s)
    _run(c, A, go, G.reference(c), unwritten)


# ===================================================================================================================== BatchNorm glue
@pytest.mark.parametrize("c", _ids(G.of("bn_finalize_fwd")))
def test_bn_finalize_fwd(c):
    dev = _dev()
    _lib, L = _mod()
    A, d, s = Arena(dev), G.inputs(c), _lib.stream()
    part, gamma, beta = A.inp("part", d["part"]), A.inp("gamma", d["gamma"]), A.inp("beta", d["beta"])
    rm, rv = A.state("run_mean", d["run_mean"]), A.state("run_var", d["run_var"])
    a, b, mean, inv = (A.out(k, c.C) for k in ("a", "b", "mean", "invstd"))

    def prepare():
        if c.run:
            rm.copy_(torch.from_numpy(d["run_mean"]))
            rv.copy_(torch.from_numpy(d["run_var"]))
    go = lambda: L.ign_bn_finalize_fwd(_p(part), c.nparts, c.nparts * c.rpp, c.C, _p(gamma), _p(beta), float(G.FIN_EPS),
                                       float(G.FIN_MOM[c.regime]), _p(rm), _p(rv), _p(a), _p(b), _p(mean), _p(inv), s)
    _run(c, A, go, G.reference(c), prepare=prepare)


@pytest.mark.parametrize("c", _ids(G.of("bn_finalize_bwd")))
def test_bn_finalize_bwd(c):
    dev = _dev()
    _lib, L = _mod()
    A, d, s = Arena(dev), G.inputs(c), _lib.stream()
    part, db, dg = A.inp("part", d["part"]), A.out("dbeta", c.C), A.out("dgamma", c.C)
    _run(c, A, lambda: L.ign_bn_finalize_bwd(_p(part), c.nparts, c.C, _p(db), _p(dg), s), G.reference(c))


@pytest.mark.parametrize("c", _ids(G.of("bn_affine_eval")))
def test_bn_affine_eval(c):
    dev = _dev()
    _lib, L = _mod()
    A, d, s = Arena(dev), G.inputs(c), _lib.stream()
    rm, rv, gamma, beta = (A.inp(k, d[k]) for k in ("run_mean", "run_var", "gamma", "beta"))
    a, b, mean, inv = (A.out(k, c.C) for k in ("a", "b", "mean", "invstd"))
    _run(c, A, lambda: L.ign_bn_affine_eval(_p(rm), _p(rv), _p(gamma), _p(beta), float(d["eps"]), c.C, _p(a), _p(b), _p(mean), _p(inv), s),
         G.reference(c))


@pytest.mark.parametrize("c", _ids(G.of("bn_relu_pool_fwd")))
def test_bn_relu_pool_fwd(c):
    """the headless entry; with a head, the head entry as well: its pooled row must be the headless one bit for bit, its logits the
    float64 product of that row"""
    dev = _dev()
    _lib, L = _mod()
    A, d, s = Arena(dev), G.inputs(c), _lib.stream()
    y, a, b = A.inp("y", d["y"]), A.inp("a", d["a"]), A.inp("b", d["b"])
    pooled = A.out("pooled", c.B, c.C)
    if c.N:
        W, bias = A.inp("W", d["W"]), A.inp("bias", d["bias"])
        pooled_h, logits = A.out("pooled_head", c.B, c.C), A.out("logits", c.B, c.N)

    def go():
        rc = L.ign_bn_relu_pool_fwd(_p(y), _p(a), _p(b), _p(pooled), c.B, c.T, c.C, s)
        if rc == 0 and c.N:
            rc = L.ign_bn_relu_pool_head_fwd(_p(y), _p(a), _p(b), _p(pooled_h), _p(W), _p(bias), _p(logits), c.B, c.T, c.C, c.N, s)
        return rc

    def late(h, first):
        if c.regime == "negative":
            h.equal("pooled is +0", bool((first["pooled"] == 0).all()))
        if c.N:
            h.equal("pooled of the head entry", torch.equal(first["pooled"], first["pooled_head"]))
            h.hold("logits", _f(first["logits"]), G.reference_pool_logits(c, d, _f(first["pooled"]).reshape(c.B, c.C)))
    _run(c, A, go, G.reference(c), late=late)


@pytest.mark.parametrize("c", _ids(G.of("bn_relu_pool_bwd")))
def test_bn_relu_pool_bwd(c):
    """g with and without the partials (equal bit for bit); the partials through ign_bn_finalize_bwd against float64 sums"""
    dev = _dev()
    _lib, L = _mod()
    A, d, s = Arena(dev), G.inputs(c), _lib.stream()
    y, gp, a, b, mean, inv = (A.inp(k, d[k]) for k in ("y", "gpool", "a", "b", "mean", "invstd"))
    pl = G.plan_pool_bwd(c.C, c.T, c.B)
    nparts = int(L.ign_bn_relu_pool_bwd_parts(c.B, c.T))
    assert nparts == pl["parts"]
    g, g_alt = A.out("g", c.B, c.T, c.C), A.out("g_alt", c.B, c.T, c.C)
    part, db, dg = A.out("part", nparts, 2, c.C), A.out("dbeta", c.C), A.out("dgamma", c.C)

    def go():
        first, second = (part, None) if c.part else (None, part)
        rc = L.ign_bn_relu_pool_bwd(_p(y), _p(gp), _p(a), _p(b), _p(mean), _p(inv), _p(g), _p(first), c.B, c.T, c.C, s)
        rc = rc or L.ign_bn_relu_pool_bwd(_p(y), _p(gp), _p(a), _p(b), _p(mean), _p(inv), _p(g_alt), _p(second), c.B, c.T, c.C, s)
        return rc or L.ign_bn_finalize_bwd(_p(part), nparts, c.C, _p(db), _p(dg), s)

    def late(h, first):
        h.equal("g without / with partials", torch.equal(first["g"], first["g_alt"]))
        sums = G.reference_pool_bwd_sums(c, d, _f(first["g"]).reshape(c.B, c.T, c.C))
        h.hold("dbeta", _f(first["dbeta"]), sums["dbeta"])
        h.hold("dgamma", _f(first["dgamma"]), sums["dgamma"])
    _run(c, A, go, G.reference(c), late=late)


@pytest.mark.parametrize("c", _ids(G.of("bn_bwd_apply")))
def test_bn_bwd_apply(c):
    dev = _dev()
    _lib, L = _mod()
    A, d, s = Arena(dev), G.inputs(c), _lib.stream()
    g, y, a, mean, inv, dbeta, dgamma = (A.inp(k, d[k]) for k in ("g", "y", "a", "mean", "invstd", "dbeta", "dgamma"))
    dyp = A.out("dyp", c.B, c.T + 2 * c.pad, c.C)
    ref = G.reference(c)
    above = np.float32(2.0 * np.abs(ref["dyp"].ref).max() + 1.0)
    slot = A.state("slot", np.zeros(1, np.float32)) if c.slot != "none" else None

    def prepare():
        if slot is not None:
            slot.fill_(float(above) if c.slot == "above" else 0.0)
    if slot is None:
        go = lambda: L.ign_bn_bwd_apply(_p(g), _p(y), _p(a), _p(mean), _p(inv), _p(dbeta), _p(dgamma), _p(dyp), c.B, c.T, c.C, c.pad, c.tr, s)
    else:
        go = lambda: L.ign_bn_bwd_apply_amax(_p(g), _p(y), _p(a), _p(mean), _p(inv), _p(dbeta), _p(dgamma), _p(dyp), _p(slot), c.B, c.T, c.C,
                                             c.pad, c.tr, s)

    def late(h, first):
        out = first["dyp"].view(torch.float32).view(c.B, c.T + 2 * c.pad, c.C)
        pads = torch.cat([out[:, :c.pad], out[:, c.pad + c.T:]], 1)
        h.equal("pad rows are 0", bool((pads == 0).all()))
        if slot is not None:
            want = torch.tensor([above], device=out.device) if c.slot == "above" else out.abs().max().reshape(1)
            h.equal(f"slot ({c.slot}) is bitwise max|dyp|" if c.slot == "zero" else "slot (above) stays",
                    torch.equal(first["slot"], want.view(torch.int32)))
    _run(c, A, go, ref, prepare=prepare, late=late)


# ===================================================================================================================== bounds
def _bits(x):
    return int(np.float32(x).view(np.uint32))


@pytest.mark.parametrize("c", _ids(G.of("absmax")))
def test_absmax_and_absmax_multi_of_one_tensor(c):
    dev = _dev()
    _lib, L = _mod()
    A, s = Arena(dev), _lib.stream()
    x_np = G.absmax_data(c.n, c.where, c.n * 7 + len(c.where))
    x = A.fenced("x", x_np)
    s1, s2 = A.state("slot", np.zeros(1, np.float32)), A.state("slot_multi", np.zeros(1, np.float32))
    want = _bits(np.abs(x_np).max())
    assert want != 0
    counts = (ctypes.c_longlong * 1)(c.n)

    def prepare():
        s1.zero_()
        s2.zero_()

    def go():
        return L.ign_absmax(_p(x), c.n, _p(s1), s) or L.ign_absmax_multi(1, _ptrs([x]), counts, _ptrs([s2]), s)

    def late(h, first):
        h.equal("ign_absmax is max|x| to the bit", int(first["slot"].view(torch.int32)[0]) & 0xFFFFFFFF == want)
        h.equal("ign_absmax_multi equals ign_absmax", torch.equal(first["slot"], first["slot_multi"]))
    _run(c, A, go, {}, prepare=prepare, late=late)


@pytest.mark.parametrize("c", _ids(G.of("absmax_multi")))
def test_absmax_multi(c):
    """up to 16 tensors of different sizes in one launch, one of them one float off alignment (the scalar route), slots pre-set to 0,
    below and above the maximum"""
    dev = _dev()
    _lib, L = _mod()
    A, s = Arena(dev), _lib.stream()
    xs_np = [G.absmax_data(n, G.ABSMAX_WHERE[i % 3], 100 * i + n) * np.float32(1 + i) for i, n in enumerate(c.sizes)]
    xs = [A.fenced(f"x{i}", x, 5 if i + 1 == c.off else 4) for i, x in enumerate(xs_np)]
    assert all((x.data_ptr() % 16 == 0) == (i + 1 != c.off) for i, x in enumerate(xs))
    mx = [float(np.abs(x).max()) for x in xs_np]
    preset = [(0.0, m / 2, 2 * m + 1)[i % 3] for i, m in enumerate(mx)]
    slots = A.state("slots", np.zeros(c.nt, np.float32))
    ref_slots = A.state("ref_slots", np.zeros(c.nt, np.float32))
    counts = (ctypes.c_longlong * c.nt)(*c.sizes)
    sp = _ptrs([slots[i:i + 1] for i in range(c.nt)])
    aligned = [i for i in range(c.nt) if i + 1 != c.off]

    def prepare():
        slots.copy_(torch.tensor(preset))
        ref_slots.zero_()

    def go():
        rc = L.ign_absmax_multi(c.nt, _ptrs(xs), counts, sp, s)
        for i in aligned:
            rc = rc or L.ign_absmax(_p(xs[i]), c.sizes[i], _p(ref_slots[i:i + 1]), s)
        return rc

    def late(h, first):
        got = first["slots"].cpu().numpy().view(np.uint32)
        h.equal("slots", [int(v) for v in got] == [_bits(max(m, p)) for m, p in zip(mx, preset)])
        one = first["ref_slots"].cpu().numpy().view(np.uint32)
        h.equal("ign_absmax on the same data", all(int(one[i]) == _bits(mx[i]) for i in aligned))
    _run(c, A, go, {}, prepare=prepare, late=late)


@pytest.mark.parametrize("c", _ids(G.of("fcn_scan")))
def test_fcn_scan(c):
    dev = _dev()
    _lib, L = _mod()
    A, d, s = Arena(dev), G.inputs(c), _lib.stream()
    w = [A.fenced(f"w{l}", x) for l, x in enumerate(d["w"])]
    gamma = [A.fenced(f"gamma{l}", x) if x is not None else None for l, x in enumerate(d["gamma"])]
    beta = [A.fenced(f"beta{l}", x) if x is not None else None for l, x in enumerate(d["beta"])]
    slots = A.out("slots", 4 * c.nl)
    zero = A.out("zero", c.nzero) if c.nzero else None
    one = A.state("absmax", np.zeros(c.nl, np.float32))
    nw, Cs, Rs = (ctypes.c_longlong * c.nl)(*c.nw), (ctypes.c_int * c.nl)(*c.C), (ctypes.c_longlong * c.nl)(*d["R"])

    def go():
        rc = L.ign_fcn_scan(c.nl, _ptrs(w), nw, _ptrs(gamma), _ptrs(beta), Cs, Rs, _p(slots), _p(zero), c.nzero, s)
        for l in range(c.nl):
            rc = rc or L.ign_absmax(_p(w[l]), c.nw[l], _p(one[l:l + 1]), s)
        return rc

    def late(h, first):
        if c.nzero:
            h.equal("zeroed", bool((first["zero"] == 0).all()))
        h.equal("slot 4l equals ign_absmax", torch.equal(first["slots"].view(-1, 4)[:, 0], first["absmax"]))
        h.equal("slots 4l + 2, 4l + 3 are +0", bool((first["slots"].view(-1, 4)[:, 2:] == 0).all()))
    _run(c, A, go, G.reference(c), prepare=lambda: one.zero_(), late=late)


# ===================================================================================================================== regularisers
@pytest.mark.parametrize("c", _ids(G.of("diversity")))
def test_diversity(c):
    dev = _dev()
    _lib, L = _mod()
    A, d, s = Arena(dev), G.inputs(c), _lib.stream()
    w, lp, gw = A.inp("w", d["w"]), A.out("loss_part", c.C), A.out("gw", c.K, c.C, c.L)

    def late(h, first):
        h.equal("finite", bool(torch.isfinite(first["loss_part"].view(torch.float32)).all() and torch.isfinite(first["gw"].view(torch.float32)).all()))
    _run(c, A, lambda: L.ign_diversity_fwd_bwd(_p(w), _p(lp), _p(gw), c.K, c.C, c.L, G.DIV_EPS, s), G.reference(c), late=late)


class _Reg:
    """one configuration of ign_sbm_reg_fwd_bwd inside an arena; the workspace comes from the caller"""

    def __init__(self, A, c, tag=""):
        _lib, L = _mod()
        self.c, d = c, G.inputs(c)
        self.W = A.inp(tag + "W", d["W"]) if c.nW else None
        self.gW = A.out(tag + "gW_reg", c.nW) if c.nW else None
        self.w = [A.inp(f"{tag}w{g}", x) for g, x in enumerate(d["w"])]
        self.gw = [A.out(f"{tag}gw{g}", *x.shape) for g, x in enumerate(d["w"])]
        self.loss = A.out(tag + "loss", 1)
        self.K = (ctypes.c_int * max(c.G, 1))(*[x.shape[0] for x in d["w"]])
        self.L = (ctypes.c_int * max(c.G, 1))(*[x.shape[2] for x in d["w"]])
        self.words = int(L.ign_sbm_reg_workspace_bytes(c.G, c.C, c.nW)) // 4
        assert self.words == G.plan_reg(c.G, c.C, c.nW)["ws_words"]

    def go(self, ws):
        _lib, L = _mod()
        c = self.c
        tabs = (_ptrs(self.w), _ptrs(self.gw), self.K, self.L) if c.G else (None, None, None, None)
        return L.ign_sbm_reg_fwd_bwd(_p(self.W), _p(self.gW), c.nW, c.lam_reg, c.G, *tabs, c.C, c.lam_div, G.DIV_EPS, _p(self.loss), _p(ws),
                                     _lib.stream())


@pytest.mark.parametrize("c", _ids(G.of("sbm_reg")))
def test_sbm_reg(c):
    """the workspace at exactly the queried size, zero-filled once: the second call runs on what the first left"""
    dev = _dev()
    A = Arena(dev)
    r = _Reg(A, c)
    ws = A.state("workspace", np.zeros(r.words, np.float32))

    def late(h, first):
        h.equal("the ticket word reads 0", int(first["workspace"][G.REG_TICKET_WORD]) == 0)
        if c.zeros:
            W = torch.from_numpy(G.inputs(c)["W"])
            h.equal("gradient at +-0 compares equal to 0", bool((first["gW_reg"].view(torch.float32).cpu()[W == 0] == 0).all()) and bool((W == 0).sum() > 100))
    _run(c, A, lambda: r.go(ws), G.reference(c), late=late)


def _case(**p):
    return G.Case("sbm_reg", "gauss", **dict(dict(lam_reg=0.3, lam_div=0.2, zeros=0), **p))


def test_sbm_reg_three_calls_of_one_configuration_on_one_workspace():
    """sequence (a): bitwise equal, the ticket word 0 afterwards"""
    dev = _dev()
    A = Arena(dev)
    r = _Reg(A, _case(**G.REG_SEQ_A))
    ws = A.state("workspace", np.zeros(r.words, np.float32))
    ref, seen = G.reference(r.c), []
    for _ in range(3):
        A.reset_outputs()
        assert r.go(ws) == 0
        torch.cuda.synchronize()
        assert A.broken_guards() == []
        assert int(A.words("workspace")[G.REG_TICKET_WORD]) == 0
        seen.append(A.outputs())
        loss = float(A.f64("loss")[0])
        assert abs(loss - ref["loss"].ref[0]) <= ref["loss"].tol[0], loss
    for o in seen[1:]:
        assert all(torch.equal(o[k], seen[0][k]) for k in o)


def test_sbm_reg_calls_of_different_sizes_share_one_workspace():
    """sequence (b): large nblk, small, large, on one buffer zero-filled once, loss_out NaN before every call: every call writes the
    right loss (a ticket behind the partials would sit on a partial of the larger call and never reach nblk - 1)"""
    dev = _dev()
    A = Arena(dev)
    regs = [_Reg(A, _case(**p), tag=f"call{i}_") for i, p in enumerate(G.REG_SEQ_B)]
    ws = A.state("workspace", np.zeros(max(r.words for r in regs), np.float32))
    h = _Holds(G.Case("sbm_reg", "sequence_b", nblk="-".join(str(G.plan_reg(**p)["nblk"]) for p in G.REG_SEQ_B)), route="three calls, one workspace")
    kept = []
    for i, r in enumerate(regs):
        A.reset_outputs()
        assert r.go(ws) == 0
        torch.cuda.synchronize()
        assert A.broken_guards() == []
        ref = G.reference(r.c)
        for k in ref:
            h.hold(f"call {i} {k}", A.f64(f"call{i}_{k}"), ref[k])
        h.equal(f"call {i} ticket word reads 0", int(A.words("workspace")[G.REG_TICKET_WORD]) == 0)
        kept.append({k: A.words(f"call{i}_{k}").clone() for k in ref})
    h.equal("first and third call", all(torch.equal(kept[0][k], kept[2][k]) for k in kept[0]))
    h.finish()


# ===================================================================================================================== refusals
@pytest.mark.parametrize("entry,what,code", [pytest.param(*r, id=f"{r[0]}-{r[1]}") for r in G.REFUSALS])
def test_refusals_return_their_codes_and_write_nothing(entry, what, code):
    """only shapes the entry point checks before it launches; every output stays as it was"""
    dev = _dev()
    _lib, L = _mod()
    A, s = Arena(dev), _lib.stream()
    z = lambda *shape: A.inp(f"in{len(A.bufs)}", np.ones(shape, np.float32))
    o = lambda *shape: A.out(f"out{len(A.bufs)}", *shape)
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    if entry in ("head_fwd", "head_bwd"):
        B, F, N, ldx = 2, 8, 3, 8
        if what == "F%4":
            F, ldx = 6, 8
        elif what == "ldx%4":
            ldx = 10
        elif what == "ldx<F":
            ldx = 4
        elif what == "N257":
            N = 257
        elif what == "B641_N16":
            B, N = 641, 16
        elif what == "B3414_N3":
            B, N = 3414, 3
        X, W, g = z(B, max(ldx, F) + 4), z(N, F + 4), z(B, N)
        Xp, Wp = (off(X) if what == "X_misaligned" else _p(X)), (off(W) if what == "W_misaligned" else _p(W))
        if entry == "head_fwd":
            rc = L.ign_head_fwd(Xp, Wp, None, _p(o(B, N)), B, F, N, ldx, s)
        else:
            rc = L.ign_head_bwd(_p(g), Xp, Wp, _p(o(B, max(ldx, F))), _p(o(N, F)), _p(o(N)), B, F, N, ldx, s)
    elif entry == "diversity":
        rc = L.ign_diversity_fwd_bwd(_p(z(17, 2, 5)), _p(o(2)), _p(o(17, 2, 5)), 17, 2, 5, G.DIV_EPS, s)
    elif entry == "sbm_reg":
        K, Gn, nW = (17 if what == "K17" else 2), (9 if what == "G9" else 0 if what == "nothing" else 1), (0 if what == "nothing" else 16)
        w, gw, ws = z(K, 2, 5), o(K, 2, 5), o(64)
        n = max(Gn, 1)
        rc = L.ign_sbm_reg_fwd_bwd(_p(z(16)), _p(o(16)), nW, 0.1, Gn, _ptrs([w] * n), _ptrs([gw] * n), (ctypes.c_int * n)(*[K] * n),
                                   (ctypes.c_int * n)(*[5] * n), 2, 0.1, G.DIV_EPS, _p(o(1)), _p(ws), s)
    elif entry.startswith("bn_"):
        C = int(what[1:])
        B, T = 2, 3
        y, v = z(B, T, C), z(C)
        if entry == "bn_relu_pool_fwd":
            rc = L.ign_bn_relu_pool_fwd(_p(y), _p(v), _p(v), _p(o(B, C)), B, T, C, s)
        elif entry == "bn_relu_pool_head_fwd":
            rc = L.ign_bn_relu_pool_head_fwd(_p(y), _p(v), _p(v), _p(o(B, C)), _p(z(3, C)), None, _p(o(B, 3)), B, T, C, 3, s)
        elif entry == "bn_relu_pool_bwd":
            rc = L.ign_bn_relu_pool_bwd(_p(y), _p(z(B, C)), _p(v), _p(v), _p(v), _p(v), _p(o(B, T, C)), _p(o(B, 2, C)), B, T, C, s)
        else:
            rc = L.ign_bn_bwd_apply_amax(_p(y), _p(y), _p(v), _p(v), _p(v), _p(v), _p(v), _p(o(B, T + 2, C)), _p(o(1)), B, T, C, 1, 1, s)
    elif entry == "absmax_multi":
        xs = [z(8)] * 17
        rc = L.ign_absmax_multi(17, _ptrs(xs), (ctypes.c_longlong * 17)(*[8] * 17), _ptrs([o(1)] * 17), s)
    elif entry == "absmax":
        rc = L.ign_absmax(off(z(12)), 8, _p(o(1)), s)
    else:
        w = [z(8)] * 9
        rc = L.ign_fcn_scan(9, _ptrs(w), (ctypes.c_longlong * 9)(*[8] * 9), None, None, None, None, _p(o(36)), None, 0, s)
    torch.cuda.synchronize()
    assert rc == code, (rc, L.ign_last_error())
    assert A.broken_guards() == []
    for name, words in A.outputs().items():
        assert bool((words == SENT).all()), f"{name} was written by a refused call"
