"""Shapelet bank, host side: the bank record (ops._Bank) and its three launchers (ops._bank_fwd, _bank_wgrad, _bank_xgrad) against
the C ABI -- which entry points are called, how often and in which order on either side of BANK_MAX_GROUPS, and every argument at the
position include/ign_abi.h gives its NAME -- plus the structure rules (one constant, entry points only in the launchers) and the
number of values ShapeletBankFn / SbmFn return from backward.  Needs neither a device nor libign_hip.so: the launchers run on CPU
tensors against a stand-in library that records the call.  The call traces asserted here were first recorded from the helpers this
layout replaced (_bank_forward / _bank_backward / _bank_backward_input), so they pin that behaviour, not this code's."""
import ast
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM = 0x5EED
L1, MSE, COS = 0, 1, 2
RBF, LTS = 0x00, 0x10
MODES = [L1 | RBF, MSE | LTS, COS | RBF]
B, C, T, EPS = 2, 3, 40, 0.75
LAUNCHERS = {"_bank_fwd", "_bank_wgrad", "_bank_xgrad"}


def _mods():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops, _lib
    return ops, _lib


# ---------------------------------------------------------------- the three directions, as the tests drive them
def _forward(ops, xn, ws, thrs, mode, strides, need_grad):
    bank = ops._Bank(xn, ws, thrs, EPS, mode, strides, need_grad)
    P, D = ops._bank_fwd(bank, xn)
    return bank, P, D


def _wgrad(ops, bank, xn, gP, P, D, gw_add=None, add_scale=None):
    return ops._bank_wgrad(bank, xn, gP, P, D, gw_add, add_scale)


def _xgrad(ops, bank, xn, gP, P, D):
    return ops._bank_xgrad(bank, xn, gP, P, D)


def _saved(bank, g):
    """-> (tstar, zmu, dsave, xstat, col0) of group g"""
    s = bank.groups[g]
    return s.tstar, s.zmu, s.dsave, s.xstat, s.col0


# ---------------------------------------------------------------- stand-in library
class _StandIn:
    """Every attribute is an entry point that records (name, args); size queries answer `nbytes`, launches 0."""

    def __init__(self, nbytes=4096):
        self.calls, self.nbytes = [], nbytes

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return self.nbytes if name.endswith("_bytes") else 0
        return fn


@pytest.fixture
def host(monkeypatch):
    ops, _lib = _mods()
    rec, labels = _StandIn(), []
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "check", lambda rc, what: labels.append(what))
    monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(STREAM))
    return ops, _lib, rec, labels


def _header_params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)", hdr)
    assert m, name
    return [re.split(r"[\s*]+", p.strip())[-1] for p in m.group(1).split(",")]


def _val(a):
    """What the C side would see: an address (None = null), a number, or -- for a host table -- the list of its entries."""
    if a is None or isinstance(a, (int, float)):
        return a
    if isinstance(a, ctypes.c_void_p):
        return a.value
    if isinstance(a, ctypes.Array):
        return list(a)
    return a.data_ptr()


def _named(_lib, call, name):
    """The recorded call as {header parameter name: value}: the entry point is `name`, it is declared in _lib.SIGNATURES, and the
    argument count is the signature's and the header's."""
    got, args = call
    assert got == name
    params = _header_params(name)
    assert name in _lib.SIGNATURES and len(args) == len(_lib.SIGNATURES[name][1]) == len(params), name
    return dict(zip(params, [_val(a) for a in args]))


def _bank(G, mode):
    """G groups: K cycles through 2..5, L = 5, 8, 11, ... (distinct), the middle group at stride 2."""
    gen = torch.Generator().manual_seed(G)
    Ks, Ls = [2 + g % 4 for g in range(G)], [5 + 3 * g for g in range(G)]
    strides = [2 if g == G // 2 else 1 for g in range(G)]
    xn = torch.randn(B, C, T, generator=gen)
    ws = [torch.randn(K, C, L, generator=gen) for K, L in zip(Ks, Ls)]
    thrs = [torch.rand(1, K, C, generator=gen) for K in Ks] if mode & LTS else [None] * G
    return xn, ws, thrs, Ks, Ls, strides


def _p(ts):
    return [None if t is None else t.data_ptr() for t in ts]


def _common(xn, P, D, Ks, mode):
    return dict(xn_bct=xn.data_ptr(), p_out=P.data_ptr(), dmin_out=D.data_ptr(), ld=sum(Ks) * C, B=B, C=C, T=T, eps=EPS, mode=mode,
                stream=STREAM)


def _col0(Ks):
    return [sum(Ks[:g]) * C for g in range(len(Ks))]


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("need_grad", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("G", [1, 4, 8, 9])
def test_forward_launcher(host, G, mode, need_grad):
    ops, _lib, rec, labels = host
    xn, ws, thrs, Ks, Ls, strides = _bank(G, mode)
    bank, P, D = _forward(ops, xn, ws, thrs, mode, strides, need_grad)
    sv = [_saved(bank, g) for g in range(G)]
    tstar, zmu, dsave, xstat, col0 = [list(f) for f in zip(*sv)]
    assert P.shape == D.shape == (B, sum(Ks) * C) and P.dtype == D.dtype == torch.float32
    assert col0 == _col0(Ks)
    for g in range(G):                                # what is allocated, and when
        Tw = (T - Ls[g]) // strides[g] + 1
        assert tstar[g].shape == (B, Ks[g], C) and tstar[g].dtype == torch.int32
        assert zmu[g].shape == (B, Ks[g], C, 2) and zmu[g].dtype == torch.float32
        assert (dsave[g] is not None) == need_grad and (xstat[g] is not None) == (need_grad and mode & 0xf == COS)
        assert dsave[g] is None or dsave[g].shape == (B, C, Ks[g], Tw)
        assert xstat[g] is None or xstat[g].shape == (B, C, Tw)
    common = _common(xn, P, D, Ks, mode)
    if G <= 8:
        (call,) = rec.calls
        assert labels == ["ign_shapelet_fwd_bank"]
        assert _named(_lib, call, "ign_shapelet_fwd_bank") == dict(
            common, G=G, w_kcl=_p(ws), thr_kc=_p(thrs), col0=col0, tstar=_p(tstar), zmu=_p(zmu), d_save=_p(dsave), xstat_save=_p(xstat),
            K=Ks, L=Ls, stride=strides)
    else:
        assert labels == ["ign_shapelet_fwd"] * G and len(rec.calls) == G
        for g, call in enumerate(rec.calls):          # group order
            assert _named(_lib, call, "ign_shapelet_fwd") == dict(
                common, w_kcl=ws[g].data_ptr(), thr_kc=_p(thrs)[g], col0=col0[g], tstar=tstar[g].data_ptr(), zmu=zmu[g].data_ptr(),
                d_save=_p(dsave)[g], xstat_save=_p(xstat)[g], K=Ks[g], L=Ls[g], stride=strides[g])


def test_channel_mismatch_keeps_its_message(host):
    ops, _lib, rec, _ = host
    xn, ws, thrs, _, _, strides = _bank(2, L1 | RBF)
    ws[1] = torch.zeros(3, C + 1, 8)
    with pytest.raises(_lib.IgnError, match=rf"^shapelet group 1: weights have {C + 1} channels, input has {C}$"):
        _forward(ops, xn, ws, thrs, L1 | RBF, strides, True)
    assert not rec.calls


# ---------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("G", [1, 4, 8, 9])
def test_weight_gradient_launcher(host, G, mode, with_add):
    ops, _lib, rec, labels = host
    xn, ws, thrs, Ks, Ls, strides = _bank(G, mode)
    bank, P, D = _forward(ops, xn, ws, thrs, mode, strides, True)
    sv = [_saved(bank, g) for g in range(G)]
    tstar, zmu, dsave, xstat, col0 = [list(f) for f in zip(*sv)]
    gP = torch.randn(B, sum(Ks) * C)
    gw_add = [torch.ones_like(w) for w in ws] if with_add else None
    scale = torch.full((1,), 0.5) if with_add else None
    del rec.calls[:], labels[:]
    gws = _wgrad(ops, bank, xn, gP, P, D, gw_add, scale)
    assert [g.shape for g in gws] == [w.shape for w in ws]
    cos = mode & 0xf == COS
    common = dict(_common(xn, P, D, Ks, mode), g_out=gP.data_ptr())
    if G <= 8:
        size, call = rec.calls
        assert labels == ["ign_shapelet_bwd_bank"]
        assert _named(_lib, size, "ign_shapelet_bwd_bank_workspace_bytes") == dict(G=G, B=B, C=C, T=T, K=Ks, L=Ls, stride=strides, mode=mode)
        got = _named(_lib, call, "ign_shapelet_bwd_bank")
        assert [p is not None for p in got.pop("wnorm_kc")] == [cos] * G and got.pop("workspace") is not None
        assert got == dict(common, G=G, w_kcl=_p(ws), col0=col0, tstar=_p(tstar), zmu=_p(zmu), d_save=_p(dsave), xstat_save=_p(xstat),
                           gw_kcl=_p(gws), gw_add=_p(gw_add) if with_add else None, add_scale_dev=scale.data_ptr() if with_add else None,
                           K=Ks, L=Ls, stride=strides)
    else:
        assert labels == ["ign_shapelet_bwd"] * G and len(rec.calls) == 2 * G
        for g in range(G):                            # per group: one size query, then one launch
            size, call = rec.calls[2 * g:2 * g + 2]
            assert _named(_lib, size, "ign_shapelet_bwd_workspace_bytes") == dict(B=B, C=C, T=T, K=Ks[g], L=Ls[g], stride=strides[g], mode=mode)
            got = _named(_lib, call, "ign_shapelet_bwd")
            assert (got.pop("wnorm_kc") is not None) == cos and got.pop("workspace") is not None
            out = got.pop("gw_kcl")                   # the regulariser's share is added by torch, into a new tensor
            assert (out != gws[g].data_ptr()) if with_add else (out == gws[g].data_ptr())
            assert got == dict(common, w_kcl=ws[g].data_ptr(), col0=col0[g], tstar=tstar[g].data_ptr(), zmu=zmu[g].data_ptr(),
                               d_save=dsave[g].data_ptr(), xstat_save=_p(xstat)[g], K=Ks[g], L=Ls[g], stride=strides[g])


@pytest.mark.parametrize("G,text", [(4, r"K=[2, 3, 4, 5] L=[5, 8, 11, 14] stride=[1, 1, 2, 1]"), (9, "K=2 L=5 stride=1")])
def test_weight_gradient_without_a_launch_plan(host, monkeypatch, G, text):
    ops, _lib, _, labels = host
    xn, ws, thrs, Ks, _, strides = _bank(G, L1 | RBF)
    bank, P, D = _forward(ops, xn, ws, thrs, L1 | RBF, strides, True)
    rec = _StandIn(nbytes=0)
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    del labels[:]
    with pytest.raises(_lib.IgnError, match="^" + re.escape("shapelet backward: no launch plan for " + text) + "$"):
        _wgrad(ops, bank, xn, torch.zeros(B, sum(Ks) * C), P, D)
    assert len(rec.calls) == 1 and rec.calls[0][0].endswith("_workspace_bytes") and not labels


# ---------------------------------------------------------------- input gradient
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("G", [1, 4, 8, 9])
def test_input_gradient_launcher(host, G, mode):
    ops, _lib, rec, labels = host
    xn, ws, thrs, Ks, Ls, strides = _bank(G, mode)
    bank, P, D = _forward(ops, xn, ws, thrs, mode, strides, True)
    sv = [_saved(bank, g) for g in range(G)]
    tstar, zmu, dsave, _, col0 = [list(f) for f in zip(*sv)]
    gP = torch.randn(B, sum(Ks) * C)
    del rec.calls[:], labels[:]
    gxn = _xgrad(ops, bank, xn, gP, P, D)
    assert gxn.shape == xn.shape and gxn.dtype == torch.float32
    common = dict(_common(xn, P, D, Ks, mode), g_out=gP.data_ptr(), gxn_bct=gxn.data_ptr())
    if G <= 8:
        (call,) = rec.calls
        assert labels == ["ign_shapelet_bwd_input_bank"]
        assert _named(_lib, call, "ign_shapelet_bwd_input_bank") == dict(
            common, G=G, w_kcl=_p(ws), col0=col0, tstar=_p(tstar), zmu=_p(zmu), d_save=_p(dsave), K=Ks, L=Ls, stride=strides)
    else:
        assert labels == ["ign_shapelet_bwd_input"] * G and len(rec.calls) == G
        for g, call in enumerate(rec.calls):          # the first group overwrites, the others add
            assert _named(_lib, call, "ign_shapelet_bwd_input") == dict(
                common, w_kcl=ws[g].data_ptr(), col0=col0[g], tstar=tstar[g].data_ptr(), zmu=zmu[g].data_ptr(),
                d_save=dsave[g].data_ptr(), accumulate=1 if g else 0, K=Ks[g], L=Ls[g], stride=strides[g])


# ---------------------------------------------------------------- structure
def _tree(*rel):
    return ast.parse(open(os.path.join(ROOT, "speech-imagery-eeg_amd", *rel)).read())


def test_shapelet_entry_points_are_named_in_the_three_launchers_only():
    users = set()
    for fn in [n for n in ast.walk(_tree("ign_hip", "ops.py")) if isinstance(n, ast.FunctionDef)]:
        for n in ast.walk(fn):
            if isinstance(n, ast.Attribute) and re.match(r"ign_shapelet_(fwd|bwd)", n.attr) and fn.name not in LAUNCHERS:
                users.add((fn.name, n.attr))
    assert not users


def test_the_group_limit_is_one_named_constant():
    """BANK_MAX_GROUPS mirrors SHP_MAX_GROUPS of csrc/ign_common.h; no comparison in ops.py or models/Shapelet.py has a literal 8."""
    ops, _ = _mods()
    src = open(os.path.join(ROOT, "speech-imagery-eeg_amd", "csrc", "ign_common.h")).read()
    assert ops.BANK_MAX_GROUPS == int(re.search(r"constexpr int SHP_MAX_GROUPS = (\d+);", src).group(1)) == 8
    for rel in (("ign_hip", "ops.py"), ("models", "Shapelet.py")):
        for n in ast.walk(_tree(*rel)):
            if isinstance(n, ast.Compare):
                lits = [c for c in [n.left] + n.comparators if isinstance(c, ast.Constant) and c.value == 8 and type(c.value) is int]
                assert not lits, (rel, n.lineno)
    names = [n.attr for n in ast.walk(_tree("models", "Shapelet.py")) if isinstance(n, ast.Attribute)]
    assert "BANK_MAX_GROUPS" in names


# ---------------------------------------------------------------- what backward returns
class _Ctx:
    """What forward / backward of an autograd.Function ask of their ctx."""

    def __init__(self, needs):
        self.needs_input_grad = needs

    def mark_non_differentiable(self, *ts):
        pass

    def set_materialize_grads(self, flag):
        pass

    def save_for_backward(self, *ts):
        self.saved_tensors = ts


@pytest.mark.parametrize("path", ["no gP", "input only", "full"])
@pytest.mark.parametrize("lts", [False, True])
@pytest.mark.parametrize("node", ["ShapeletBankFn", "SbmFn"])
def test_backward_returns_one_value_per_forward_input(host, monkeypatch, node, lts, path):
    ops, _lib, rec, labels = host
    monkeypatch.setattr(ops, "_need_gpu", lambda name, *ts: None)
    G, mode = 3, (L1 | LTS) if lts else (L1 | RBF)
    xn, ws, thrs, Ks, _, strides = _bank(G, mode)
    params = ws + (thrs if lts else [])
    need_x, need_p = path != "full", path != "input only"
    if node == "ShapeletBankFn":
        inputs = (xn, EPS, mode, tuple(strides), G, *params)
        needs = (need_x, False, False, False, False) + (need_p,) * len(params)
    else:
        W = torch.zeros(4, sum(Ks) * C)
        cfg = (EPS, mode, tuple(strides), G, 0.1, 0.1, False, True, torch.zeros(64))
        inputs = (xn, cfg, W, *params)
        needs = (need_x, False, need_p) + (need_p,) * len(params)
    fn, ctx = getattr(ops, node), _Ctx(needs)
    outs = fn.forward(ctx, *inputs)
    P = outs[0]
    grads = [None if path == "no gP" else torch.ones_like(P)] + [None] * (len(outs) - 1)
    if node == "SbmFn":
        grads[3] = torch.ones(1)                      # the regulariser's upstream gradient
    del rec.calls[:]
    got = fn.backward(ctx, *grads)
    assert isinstance(got, tuple) and len(got) == len(inputs)
    ran = {name for name, _ in rec.calls}
    assert ran == {"no gP": set(), "input only": {"ign_shapelet_bwd_input_bank"},
                   "full": {"ign_shapelet_bwd_bank_workspace_bytes", "ign_shapelet_bwd_bank"}}[path]
    gx, gparams = got[0], got[len(inputs) - len(params):]
    assert (gx is not None) == (path == "input only")
    if path == "full":
        assert [g.shape for g in gparams] == [p.shape for p in params]
    elif path == "input only" or node == "ShapeletBankFn":
        assert all(g is None for g in gparams)
    else:                                             # SbmFn without gP: the diversity regulariser still moves the shapelets
        assert [g.shape for g in gparams[:G]] == [w.shape for w in ws] and all(g is None for g in gparams[G:])
