"""The convolution and dense GEMM kernels (csrc/ign_clconv_f32.hip, ign_clconv_x6.hip) through the C ABI at every tile, tap and split
edge of tests/conv_edge_cases.py, under every arithmetic that runs them, against float64 (tests/test_conv_edges_host.py proves what
the table covers and what the tolerance can see).

Every buffer a kernel touches is a view inside an arena whose every other word is a NaN with a payload of its own: outputs (y, the
statistics partials, g_in, gx, dw, db, the workspace at exactly the queried size) are prefilled with it, inputs are surrounded by
it -- the activations, gradients, weights, affine vectors, the f16x3 bound slots, and the packed weights, which the pack kernels
write into NaN-prefilled views of exactly the queried size before the GEMM reads them.  Each case asserts: the words around every view are bitwise intact; every output element was written; every element is within
u * tol * sum|a||b| of float64 (the bf16 route: of the float64 product of the rounded operands); the statistics partials match the
float64 sums of the kernel's own outputs to the worst-case fp32 summation bound; a second call repeats the first bit for bit.
Every figure is printed and recorded before anything is asserted; IGN_CONV_EDGES_OUT=<file> writes the record as JSON
(tests/diag_conv_edges.py -> profiles/conv_edges.json)."""
import ctypes
import json
import math
import os

import pytest
import torch

import conv_edge_cases as C

pytestmark = pytest.mark.gpu

GUARD = 256                       # words in front of and behind every view
SENT = 0x7FC5A5A5                 # a quiet NaN no kernel produces
SENT16 = 0x7FC5                   # the same for 16-bit planes: a NaN as bf16 and as fp16 (two of them: a float32 NaN as well)
X6_PLANE_ELEMS = C.TN * C.KC      # 16-bit elements per plane of one packed (n-tile, chunk, tap) block; three planes per block
_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("IGN_CONV_EDGES_OUT")
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


_V1, _I1 = ctypes.c_void_p * 1, ctypes.c_int * 1


class _Case:
    """The comparisons of one case: each is printed and recorded before anything is asserted."""

    def __init__(self, kernel, arith, case):
        self.name, self.bad = f"{kernel} {arith} {case.kind} {case.name}", []
        self.rec = _RECORD.setdefault(kernel, {}).setdefault(arith, {}).setdefault(case.regime, {}).setdefault(f"{case.kind} {case.name}", {})

    def hold(self, what, err, tol, **more):
        r = dict(err=err, tol=tol, ratio=(err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))), **more)
        self.rec[what] = r
        print(f"{self.name}: {what} {r}")
        if not err <= tol:
            self.bad.append((what, r))

    def finish(self):
        assert not self.bad, f"{self.name}: {self.bad}"


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

    def out16(self, name, n):
        """n 16-bit elements (packed operand planes), every one of them and of the surroundings SENT16"""
        assert n % 2 == 0
        buf = torch.full((2 * GUARD + n // 2,), SENT16 << 16 | SENT16, dtype=torch.int32, device=self.dev)
        self.bufs.append([name, buf, n // 2, True, None])
        return buf[GUARD:GUARD + n // 2].view(torch.int16)

    def freeze(self, name):
        """an output of the preparation (packed weights) becomes an input of the call under test: from here on it must not change"""
        rec = next(r for r in self.bufs if r[0] == name)
        rec[3], rec[4] = False, rec[1][GUARD:GUARD + rec[2]].clone()

    def inp(self, name, t):
        v = self._view(name, tuple(t.shape), False)
        v.copy_(t)
        self.bufs[-1][4] = self.words(name).clone()
        return v

    def reset_outputs(self):
        for _, buf, n, is_out, _ in self.bufs:
            if is_out:
                buf[GUARD:GUARD + n] = SENT

    def broken_guards(self):
        """the views whose surroundings changed, and the inputs that did (bitwise)"""
        bad = [name for name, buf, n, _, _ in self.bufs
               if not (bool((buf[:GUARD] == buf[0]).all()) and bool((buf[GUARD + n:] == buf[0]).all()) and int(buf[0]) in (SENT, SENT16 << 16 | SENT16))]
        return bad + [name + " (input overwritten)" for name, buf, n, _, was in self.bufs
                      if was is not None and not torch.equal(buf[GUARD:GUARD + n], was)]

    def words(self, name):
        buf, n = next((b, n) for nm, b, n, _, _ in self.bufs if nm == name)
        return buf[GUARD:GUARD + n]

    def outputs(self):
        return {name: buf[GUARD:GUARD + n].clone() for name, buf, n, is_out, _ in self.bufs if is_out}


def _pack(_lib, L, A, arith, w, Co, Ci, k, bound_w):
    """-> (forward weights, data-gradient weights) as the arithmetic's kernels read them, each a view inside the arena at exactly
    the queried size, prefilled with NaNs as production's torch.empty may be: the pack has to write every element the kernels read
    -- the zero rows past N and channels past C included -- and nothing else.  The two-plane fp16 pack leaves plane 2 of every block
    untouched by contract; it stays NaN here, so a kernel that read it would show."""
    s = _lib.stream()
    if arith == "f32":
        wt, wd = A.out("wt", Co, k * Ci), A.out("wd", Ci, k * Co)
        _lib.check(L.ign_clconv_pack_weights(_p(w), _p(wt), _p(wd), Co, Ci, k, s), "pack")
        torch.cuda.synchronize()
        for name in ("wt", "wd"):
            assert not bool((A.words(name) == SENT).any()), f"{name}: the pack left elements unwritten"
            A.freeze(name)
        assert A.broken_guards() == []
        return wt, wd
    wt, wd = A.out16("wt", int(L.ign_clconv_x3_elems(Co, Ci, k))), A.out16("wd", int(L.ign_clconv_x3_elems(Ci, Co, k)))
    if arith == "f16x3":
        _lib.check(L.ign_clconv_pack_weights_h2_multi(1, _V1(w.data_ptr()), _V1(wt.data_ptr()), _V1(wd.data_ptr()), _I1(Co), _I1(Ci), _I1(k),
                                                      None, _V1(bound_w.data_ptr()), s), "pack_h2")
    else:
        _lib.check(L.ign_clconv_pack_weights_x3(_p(w), _p(wt), _p(wd), Co, Ci, k, s), "pack_x3")
    torch.cuda.synchronize()
    for name, t in (("wt", wt), ("wd", wd)):
        unwritten = (t == SENT16).view(-1, 3, X6_PLANE_ELEMS)                  # (block, plane, 128 rows x 16 channels)
        if arith == "f16x3":
            assert not bool(unwritten[:, :2].any()), f"{name}: the pack left elements of planes 0 / 1 unwritten"
            assert bool(unwritten[:, 2].all()), f"{name}: the two-plane pack wrote plane 2"
        else:
            assert not bool(unwritten.any()), f"{name}: the pack left elements unwritten"
        A.freeze(name)
    assert A.broken_guards() == []
    return wt, wd


def _padded(dy, pad):
    B, Tout, Co = dy.shape
    out = torch.zeros(B, Tout + 2 * pad, Co)
    out[:, pad:pad + Tout] = dy
    return out


def _poison(t, keep):
    """every sample but `keep` NaN"""
    if keep is None:
        return t
    out = torch.full_like(t, float("nan"))
    out[keep] = t[keep]
    return out


class Launch:
    """One case under one arithmetic: arenas, packed weights, and `go()` -> return code of the entry point(s).
    `written`: output name -> leading words the call must have written (the whole view unless stated)."""

    def __init__(self, case, arith, dev, keep_sample=None, refuse=False):
        _lib, L = _mod()
        self.case, self.arith, self.A = case, arith, Arena(dev)
        A, d, s = self.A, C.inputs(case), _lib.stream()
        B, Tin, Ci, Co, k = case.B, case.Tin, case.Ci, case.Co, case.k
        Tout = Tin - k + 1
        h3 = arith == "f16x3"
        # f16x3 bounds: [the b operand (weights, or dy of a weight gradient), the a operand]
        slots = A.inp("bounds", torch.tensor([d["bound_b"], d["bound_a"]], dtype=torch.float32))
        bb, ba = ctypes.c_void_p(slots.data_ptr()), ctypes.c_void_p(slots.data_ptr() + 4)
        self.keep = ()
        opt = lambda name: A.inp(name, d[name]) if name in d else None
        self.written, self.plan = {}, None if refuse else C.plan_of(arith, case)
        sfx = {"f32": "", "bf16x6": "_x6", "bf16": "_bf16", "f16x3": "_h3"}[arith]
        if case.kind in ("fwd", "dgrad", "dgrad_input", "gelu"):
            w = A.inp("w", d["w"])
            wt, wd = _pack(_lib, L, A, arith, w, Co, Ci, k, slots)
            self.keep += (wt, wd)
            rows = C.dims(case)[0]
            mtiles = int(L.ign_clconv_mtiles(B * rows) if arith == "f32" else L.ign_clconv_x6_mtiles(B, rows))
        if case.kind == "fwd":
            x, bias, pa, pb = A.inp("x", _poison(d["x"], keep_sample)), A.inp("bias", d["bias"]), opt("pa"), opt("pb")
            y = A.out("y", B, Tout, Co)
            part = A.out("part", mtiles, 2, Co) if case.part else None
            fn = getattr(L, "ign_clconv_fwd" + sfx)
            tail = (ba, bb) if h3 else ()
            self.go = lambda: fn(_p(x), _p(wt), _p(bias), _p(pa), _p(pb), _p(y), _p(part), *tail, B, Tin, Ci, Co, k, s)
        elif case.kind == "dgrad":
            dyp = A.inp("dyp", _poison(_padded(d["dy"], k - 1), keep_sample))
            y_in = A.inp("y_in", _poison(d["y_in"], keep_sample))
            ea, eb, em, ei = (A.inp(n, d[n]) for n in ("ea", "eb", "emean", "einv"))
            g = A.out("g_in", B, Tin, Ci)
            part = A.out("part", mtiles, 2, Ci) if case.part else None
            fn = getattr(L, "ign_clconv_dgrad" + sfx)
            tail = (ba, bb) if h3 else ()
            self.go = lambda: fn(_p(dyp), _p(wd), _p(y_in), _p(ea), _p(eb), _p(em), _p(ei), _p(g), _p(part), *tail, B, Tin, Ci, Co, k, s)
        elif case.kind == "dgrad_input":
            dyp = A.inp("dyp", _poison(_padded(d["dy"], k - 1), keep_sample))
            gx = A.out("gx", B, Tin, Ci)
            fn = getattr(L, "ign_clconv_dgrad_input" + sfx)
            tail = (ba, bb) if h3 else ()
            self.go = lambda: fn(_p(dyp), _p(wd), _p(gx), *tail, B, Tin, Ci, Co, k, s)
        elif case.kind == "gelu":
            g, u = A.inp("g", d["dy"][0]), A.inp("u", d["u"][0])
            du = A.out("du", Tin, Ci)
            self.go = lambda: L.ign_linear_dgrad_gelu_h3(_p(g), _p(wd), _p(u), _p(du), ba, bb, None, Tin, Co, Ci, s)
        else:
            f32 = arith == "f32"
            k1 = case.kind == "wgrad_k1"
            query = L.ign_clconv_wgrad_workspace_bytes if f32 else L.ign_clconv_wgrad_x6_workspace_bytes
            nws = int(query(B, Tin, Ci, Co, k)) // 4
            if refuse:
                assert nws == 0
                nws = 64
            else:
                assert nws == self.plan["ws_floats"], "the workspace query and the restated planner disagree"
            pad = 0 if k1 else k - 1
            dyp, x, pa, pb = A.inp("dyp", _padded(d["dy"], pad)), A.inp("x", d["x"]), opt("pa"), opt("pb")
            ws, dw = A.out("ws", nws), A.out("dw", Co, Ci, k)
            db = A.out("db", Co) if case.db and not f32 else None
            if not refuse:
                self.written["ws"] = self.plan["part_floats"] + (self.plan["nsplit"] * Co if db is not None else 0)
            if k1 and not f32:
                fn = getattr(L, "ign_linear_wgrad" + sfx)
                tail = (bb, ba) if h3 else ()                       # (bound_dy, bound_x)
                self.go = lambda: fn(_p(dyp), _p(x), _p(dw), _p(db), _p(ws), *tail, B * Tin, Ci, Co, s)
            else:
                fn = getattr(L, "ign_clconv_wgrad" + sfx)
                tail = (bb, ba) if h3 else ()
                defer = case.defer and not f32
                nsplit = None if refuse or f32 else self.plan["nsplit"]

                def go():
                    rc = fn(_p(dyp), pad, _p(x), _p(pa), _p(pb), None if defer else _p(dw), _p(ws), *tail, B, Tin, Ci, Co, k, s)
                    if rc == 0 and defer:                           # partials only, then the reduction of "several layers"
                        rc = L.ign_clconv_wgrad_reduce_multi(1, _V1(ws.data_ptr()), _V1(dw.data_ptr()), _I1(nsplit), _I1(Co), _I1(Ci), _I1(k), s)
                    return rc
                self.go = go

    def run(self):
        rc = self.go()
        torch.cuda.synchronize()
        return rc


def _ratio(got, r):
    """max over the elements of |got - ref| / (u * (tol * cond + extra)); an element without a scale must be exact"""
    den = C.U * (r.tol * r.cond + r.extra)
    diff = (got - r.ref).abs()
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
    q = torch.where(den > 0, diff / den.clamp_min(1e-300), torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, float("inf"))))
    return float(q.max())


def _hold_partials(c, case, plan, d, out, part):
    """part (mtiles, 2, N) against float64 sums of the kernel's OWN outputs over each tile's rows: an fp32 sum of n terms in any
    order is within (n - 1) u sum|term| of the exact one, the terms themselves carry at most three roundings"""
    N = out.shape[-1]
    v = out.double().reshape(-1, N)
    if case.kind == "fwd":
        t1, t2 = v, v * v
    else:
        yhat = (d["y_in"].double().reshape(-1, N) - d["emean"].double()) * d["einv"].double()
        t1, t2 = v, v * yhat
    worst = [0.0, 0.0]
    for mt, (r0, r1) in enumerate(plan["tiles"]):
        for i, t in enumerate((t1, t2)):
            ref, scale = t[r0:r1].sum(0), t[r0:r1].abs().sum(0)
            den = C.U * (r1 - r0 + 4) * scale
            diff = (part[mt, i].double() - ref).abs()
            diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
            q = torch.where(den > 0, diff / den.clamp_min(1e-300), torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, float("inf"))))
            worst[i] = max(worst[i], float(q.max()))
    c.hold("partials s1", worst[0], 1.0)
    c.hold("partials s2", worst[1], 1.0)


_RUNS = [pytest.param(c, a, id=f"{c.kind}-{c.name}-{a}") for c, a in C.runs()]


@pytest.mark.parametrize("case,arith", _RUNS)
def test_edge_case_vs_float64(case, arith):
    dev = _dev()
    run = Launch(case, arith, dev)
    assert run.run() == 0, _mod()[1].ign_last_error()
    A, plan, d = run.A, run.plan, C.inputs(case)
    c = _Case(plan["kernel"], arith, case)
    assert A.broken_guards() == [], "written outside a view"
    first = A.outputs()
    for name, words in first.items():
        n = run.written.get(name, words.numel())
        unwritten = int((words[:n] == SENT).sum())
        assert unwritten == 0, f"{name}: {unwritten} of {n} elements never written"
    ref = C.reference(case, arith)
    if arith == "f32":
        ref.pop("db", None)                                           # the fp32 entry point has no bias gradient
    bd = C.bound(case, arith)
    for name, r in ref.items():
        got = first[name].view(torch.float32).double().cpu().view(r.ref.shape)
        ratio = _ratio(got, r)
        c.hold(name, ratio * r.tol, r.tol, e_model=bd.e_model, e_acc=bd.e_acc, K=bd.K)
    if "part" in first:
        name = "y" if case.kind == "fwd" else "g_in"
        N = ref[name].ref.shape[-1]
        _hold_partials(c, case, plan, d, first[name].view(torch.float32).cpu().view(ref[name].ref.shape),
                       first["part"].view(torch.float32).cpu().view(-1, 2, N))
    A.reset_outputs()
    assert run.run() == 0
    again = A.outputs()
    assert A.broken_guards() == []
    for name in first:
        assert torch.equal(first[name], again[name]), f"{name}: the second call is not a bitwise repeat"
    c.finish()


_REFUSED = [pytest.param(c, a, id=f"{c.kind}-{c.name}-{a}") for c in C.CASES for a in C.refused_ariths(c)]


@pytest.mark.parametrize("case,arith", _REFUSED)
def test_split_entry_points_refuse_what_they_cannot_run(case, arith):
    """more than 16 taps (the staged span holds TM + 15 rows), or a weight gradient whose tap count has no split kernel:
    IGN_E_UNSUP, and not one word of any output touched"""
    dev = _dev()
    run = Launch(case, arith, dev, refuse=True)
    assert run.run() == C.IGN_E_UNSUP
    assert run.A.broken_guards() == []
    for name, words in run.A.outputs().items():
        assert bool((words == SENT).all()), f"{name} was written by a refused call"


_POISON = [("fwd", "B5-T52-Ci6-Co64-k3"), ("dgrad", "B5-T50-Ci64-Co6-k3"), ("fwd", "B9-T257-Ci17-Co4-k1-pro"),
           ("dgrad", "B2-T127-Ci4-Co2-k2"), ("dgrad_input", "B2-T127-Ci1-Co4-k3")]


@pytest.mark.parametrize("arith", C.ARITHS)
@pytest.mark.parametrize("kind,name", _POISON)
def test_a_sample_does_not_see_the_other_samples(kind, name, arith):
    """every other sample's input NaN: the sample's rows equal the clean run's bit for bit (the fp32 kernel's tiles hold rows of
    several samples, the split kernels clamp their span loads inside the sample).  The forward and data-gradient kernels only: the
    wide-tile kernel takes one sample by its launch rule, and a weight gradient sums over all of them."""
    dev = _dev()
    case = C.find(kind, name)
    out = {"fwd": "y", "dgrad": "g_in", "dgrad_input": "gx"}[kind]
    clean = Launch(case, arith, dev)
    assert clean.run() == 0
    want = clean.A.words(out).view(case.B, -1)
    for keep in (1, case.B - 1):
        run = Launch(case, arith, dev, keep_sample=keep)
        assert run.run() == 0
        got = run.A.words(out).view(case.B, -1)
        assert torch.equal(got[keep], want[keep]), f"sample {keep} changed with its neighbours' inputs"
        assert run.A.broken_guards() == []
