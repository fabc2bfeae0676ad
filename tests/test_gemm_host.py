"""Dense-layer / convolution GEMMs, host side: which arithmetic and which weight-gradient kernel run (ops._dense_arith,
fcn._fcn_arith, ops._linear_wgrad_split, ops._conv_wgrad_route, fcn._wgrad_arith) against literal tables, and every launcher of
ign_hip/ops.py against the C ABI: entry point, argument count and order, the position of the fp16 path's bound arguments as
include/ign_abi.h declares them, and the name an IgnError would carry.  Needs neither a device nor libign_hip.so: the launchers run
against a stand-in library that records the call."""
import ast
import ctypes
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM = 0x5EED


def _mods():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops, fcn, _lib
    return ops, fcn, _lib


# ---------------------------------------------------------------- the rules

# (GEMM_MATH, autocast) -> arithmetic of linear / gelu_linear / conv1d_cl / the LayerNorm bound hooks / prepare_linear_weights
_DENSE_TABLE = {("f16x3", False): "H3", ("f16x3", True): "BF16", ("bf16x6", False): "X6", ("bf16x6", True): "BF16"}

# (math, every block on batch statistics, blocks) -> arithmetic of the FCN body; `math` is fcn_body's argument, or CONV_MATH outside
# an autocast region when the argument is None (inside one a None argument means "bf16")
_FCN_TABLE = {
    ("f16x3", True, 3): "H3", ("f16x3", True, 9): "X6", ("f16x3", False, 3): "X6", ("f16x3", False, 9): "X6",
    ("bf16x6", True, 3): "X6", ("bf16x6", True, 9): "X6", ("bf16x6", False, 3): "X6", ("bf16x6", False, 9): "X6",
    ("bf16", True, 3): "BF16", ("bf16", True, 9): "BF16", ("bf16", False, 3): "BF16", ("bf16", False, 9): "BF16",
    ("f32", True, 3): "F32", ("f32", True, 9): "F32", ("f32", False, 3): "F32", ("f32", False, 9): "F32",
}

# (LINEAR_WGRAD, Ci) -> ops.linear's weight gradient on the split kernel (else fp32 ign_clconv_wgrad, k = 1)
_LINEAR_WGRAD_TABLE = {("bf16x6", 8): True, ("bf16x6", 6): False, ("f32", 8): False, ("f32", 6): False}

# (LINEAR_WGRAD, k, Ci) -> conv1d_cl's weight gradient: multi-tap split kernel / one linear weight gradient per tap / fp32 kernel
_CONV_WGRAD_TABLE = {
    ("bf16x6", 1, 6): "f32", ("bf16x6", 1, 8): "f32", ("bf16x6", 2, 6): "split", ("bf16x6", 2, 8): "split",
    ("bf16x6", 4, 6): "f32", ("bf16x6", 4, 8): "taps", ("bf16x6", 7, 6): "f32", ("bf16x6", 7, 8): "taps",
    ("f32", 1, 6): "f32", ("f32", 1, 8): "f32", ("f32", 2, 6): "f32", ("f32", 2, 8): "f32",
    ("f32", 4, 6): "f32", ("f32", 4, 8): "f32", ("f32", 7, 6): "f32", ("f32", 7, 8): "f32",
}

# arithmetic of the FCN body -> arithmetic of a block's weight gradient at k = 1, 2, 3, 4, 5, 7, 8
_FCN_WGRAD_TABLE = {
    "F32": "F32 F32 F32 F32 F32 F32 F32",
    "X6": "F32 X6 X6 F32 X6 F32 X6",
    "BF16": "F32 BF16 BF16 F32 BF16 F32 BF16",
    "H3": "F32 H3 H3 F32 H3 F32 H3",
}


def test_arithmetic_constants_are_four_distinct_values():
    ops, _, _ = _mods()
    assert len({ops.GEMM_F32, ops.GEMM_X6, ops.GEMM_BF16, ops.GEMM_H3}) == 4


def test_dense_arithmetic_rule(monkeypatch):
    ops, _, _ = _mods()
    for (gemm_math, autocast), want in _DENSE_TABLE.items():
        monkeypatch.setattr(ops, "GEMM_MATH", gemm_math)
        assert ops._dense_arith(autocast) == getattr(ops, "GEMM_" + want), (gemm_math, autocast)


def test_fcn_arithmetic_rule(monkeypatch):
    ops, fcn, _ = _mods()
    for (math, all_batch, nl), want in _FCN_TABLE.items():
        states = [types.SimpleNamespace(use_batch_stats=True) for _ in range(nl)]
        states[1].use_batch_stats = all_batch
        want = getattr(ops, "GEMM_" + want)
        for autocast in (False, True):
            monkeypatch.setattr(fcn, "CONV_MATH", "no such arithmetic")          # an explicit argument wins over both
            assert fcn._fcn_arith(math, autocast, states) == want, (math, all_batch, nl, autocast)
            monkeypatch.setattr(fcn, "CONV_MATH", math)
            got = fcn._fcn_arith(None, autocast, states)
            assert got == (ops.GEMM_BF16 if autocast else want), (math, all_batch, nl, autocast)
    monkeypatch.setattr(fcn, "CONV_MATH", "no such arithmetic")                  # as before: an unknown name runs fp32 MFMA
    assert fcn._fcn_arith(None, False, states) == ops.GEMM_F32


def test_weight_gradient_rules(monkeypatch):
    ops, fcn, _ = _mods()
    for (lw, Ci), want in _LINEAR_WGRAD_TABLE.items():
        monkeypatch.setattr(ops, "LINEAR_WGRAD", lw)
        assert bool(ops._linear_wgrad_split(Ci)) is want, (lw, Ci)
    for (lw, k, Ci), want in _CONV_WGRAD_TABLE.items():
        monkeypatch.setattr(ops, "LINEAR_WGRAD", lw)
        assert ops._conv_wgrad_route(k, Ci) == want, (lw, k, Ci)
    for arith, row in _FCN_WGRAD_TABLE.items():
        for k, want in zip((1, 2, 3, 4, 5, 7, 8), row.split()):
            assert fcn._wgrad_arith(getattr(ops, "GEMM_" + arith), k) == getattr(ops, "GEMM_" + want), (arith, k)


def test_each_knob_is_read_in_one_place_and_gemm_entry_points_only_in_the_launchers():
    """GEMM_MATH is read by ops._dense_arith alone and CONV_MATH by fcn._fcn_arith alone; outside the launchers neither file touches a
    forward / data-gradient / weight-gradient GEMM entry point (the size / split-count / deferred-reduction helpers excepted)."""
    launchers = {"_clconv_fwd", "_clconv_dgrad", "_clconv_wgrad", "_linear_wgrad", "_wgrad_workspace"}
    gemm = re.compile(r"^ign_(clconv_(fwd|dgrad|wgrad)|linear_wgrad)(?!\w*(_workspace_bytes|_nsplit|_reduce_multi)$)")
    readers, users = {}, set()
    for mod in ("ops", "fcn"):
        tree = ast.parse(open(os.path.join(ROOT, "speech-imagery-eeg_amd", "ign_hip", mod + ".py")).read())
        for fn in [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]:
            for n in ast.walk(fn):
                if isinstance(n, ast.Name) and n.id in ("GEMM_MATH", "CONV_MATH"):
                    readers.setdefault(n.id, set()).add(fn.name)
                if isinstance(n, ast.Attribute) and gemm.match(n.attr) and fn.name not in launchers:
                    users.add((mod, fn.name, n.attr))
    assert readers == {"GEMM_MATH": {"_dense_arith"}, "CONV_MATH": {"_fcn_arith"}}
    assert not users


# ---------------------------------------------------------------- the launchers

_FWD = {"F32": "ign_clconv_fwd", "X6": "ign_clconv_fwd_x6", "BF16": "ign_clconv_fwd_bf16", "H3": "ign_clconv_fwd_h3"}
_DGRAD = {"F32": "ign_clconv_dgrad", "X6": "ign_clconv_dgrad_x6", "BF16": "ign_clconv_dgrad_bf16", "H3": "ign_clconv_dgrad_h3"}
_WGRAD = {"F32": "ign_clconv_wgrad", "X6": "ign_clconv_wgrad_x6", "BF16": "ign_clconv_wgrad_bf16", "H3": "ign_clconv_wgrad_h3"}
_LWGRAD = {"X6": "ign_linear_wgrad_x6", "BF16": "ign_linear_wgrad_bf16", "H3": "ign_linear_wgrad_h3"}
_WS_BYTES = {"F32": "ign_clconv_wgrad_workspace_bytes", "X6": "ign_clconv_wgrad_x6_workspace_bytes",
             "BF16": "ign_clconv_wgrad_x6_workspace_bytes", "H3": "ign_clconv_wgrad_x6_workspace_bytes"}
_PACK = {"F32": "ign_clconv_pack_weights", "X6": "ign_clconv_pack_weights_x3", "BF16": "ign_clconv_pack_weights_x3",
         "H3": "ign_clconv_pack_weights_h2_multi"}


class _StandIn:
    """Every attribute is an entry point that records (name, args); size queries answer 4096, launches 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 4096 if name.endswith(("_bytes", "_elems")) else 0
        return fn


@pytest.fixture
def host(monkeypatch):
    ops, _, _lib = _mods()
    rec, labels = _StandIn(), []
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "check", lambda rc, what: labels.append(what))
    monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(STREAM))
    return ops, _lib, rec, labels


def _header_params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
    assert m, name
    return [re.split(r"[\s*]+", p.strip())[-1] for p in m.group(1).split(",")]


def _val(a):
    if a is None or isinstance(a, int):
        return a
    return a.value if isinstance(a, ctypes.c_void_p) else a.data_ptr()


def _check_launch(_lib, call, labels, name, head, dims, bounds):
    """`call` is the one launch recorded: the entry point is `name`, declared and bound; the arguments named bound_* / amax_out in
    the header are `bounds`, in order; the others are head + dims + stream, in order; the label handed to _lib.check is the name."""
    got, args = call
    assert got == name and labels == [name]
    assert name in _lib.SIGNATURES and len(args) == len(_lib.SIGNATURES[name][1])
    params = _header_params(name)
    assert len(params) == len(args)
    bpos = [i for i, p in enumerate(params) if p.startswith("bound_") or p == "amax_out"]
    assert [_val(args[i]) for i in bpos] == [_val(b) for b in bounds], (name, params)
    assert [_val(a) for i, a in enumerate(args) if i not in bpos] == [_val(h) for h in head] + list(dims) + [STREAM], (name, params)


def _tensors(n):
    import torch
    return [torch.zeros(8) for _ in range(n)]


B1, B2 = ctypes.c_void_p(0xB10), ctypes.c_void_p(0xB20)
DIMS = (2, 10, 4, 8, 3)


@pytest.mark.parametrize("arith", ["F32", "X6", "BF16", "H3", "H3 amax"])
def test_forward_launcher(host, arith):
    ops, _lib, rec, labels = host
    x, wt, bias, pa, pb, y, part, slot = _tensors(8)
    h3, amax = arith.startswith("H3"), (slot if arith == "H3 amax" else None)
    ops._clconv_fwd(getattr(ops, "GEMM_" + arith.split()[0]), x, wt, bias, pa, None, y, part, DIMS, B1, B2, amax)
    name = "ign_clconv_fwd_h3_amax" if amax is not None else _FWD[arith]
    bounds = ([B1, B2] + ([slot] if amax is not None else [])) if h3 else []
    (call,) = rec.calls
    _check_launch(_lib, call, labels, name, [x, wt, bias, pa, None, y, part], DIMS, bounds)
    if h3:                                            # where include/ign_abi.h puts them: behind stat_part, in front of B
        assert _header_params(name)[7:9] == ["bound_in", "bound_w"]


@pytest.mark.parametrize("arith", ["F32", "X6", "BF16", "H3"])
def test_data_gradient_launcher(host, arith):
    ops, _lib, rec, labels = host
    ts = _tensors(9)
    ops._clconv_dgrad(getattr(ops, "GEMM_" + arith), *ts, DIMS, B1, B2)
    (call,) = rec.calls
    _check_launch(_lib, call, labels, _DGRAD[arith], ts, DIMS, [B1, B2] if arith == "H3" else [])
    if arith == "H3":
        assert _header_params(_DGRAD[arith])[9:11] == ["bound_dy", "bound_w"]


@pytest.mark.parametrize("arith", ["F32", "X6", "BF16", "H3"])
def test_convolution_weight_gradient_launcher(host, arith):
    ops, _lib, rec, labels = host
    dyp, x, pa, pb, dw = _tensors(5)
    ws = ops._clconv_wgrad(getattr(ops, "GEMM_" + arith), dyp, 2, x, pa, pb, dw, DIMS, B1, B2)
    size, call = rec.calls
    assert size == (_WS_BYTES[arith], DIMS) and ws.numel() == 1024 and str(ws.dtype) == "torch.float32"
    _check_launch(_lib, call, labels, _WGRAD[arith], [dyp, 2, x, pa, pb, dw, ws], DIMS, [B1, B2] if arith == "H3" else [])
    if arith == "H3":
        assert _header_params(_WGRAD[arith])[7:9] == ["bound_dy", "bound_x"]


@pytest.mark.parametrize("arith", ["X6", "BF16", "H3"])
@pytest.mark.parametrize("own_ws", [False, True])
def test_linear_weight_gradient_launcher(host, arith, own_ws):
    ops, _lib, rec, labels = host
    dy, x, dw, db, ws = _tensors(5)
    M, Ci, Co = 40, 4, 8
    ops._linear_wgrad(getattr(ops, "GEMM_" + arith), dy, x, dw, db if own_ws else None, M, Ci, Co, B1, B2, ws if own_ws else None)
    if not own_ws:
        assert rec.calls[0] == ("ign_clconv_wgrad_x6_workspace_bytes", (1, M, Ci, Co, 1))
        ws = rec.calls[-1][1][4]                      # the workspace the launcher allocated: only its position can be checked
    assert len(rec.calls) == (1 if own_ws else 2)
    _check_launch(_lib, rec.calls[-1], labels, _LWGRAD[arith], [dy, x, dw, db if own_ws else None, ws], (M, Ci, Co),
                  [B1, B2] if arith == "H3" else [])
    if arith == "H3":
        assert _header_params(_LWGRAD[arith])[5:7] == ["bound_dy", "bound_x"]


@pytest.mark.parametrize("arith", ["F32", "X6", "BF16", "H3"])
@pytest.mark.parametrize("need_dx", [False, True])
def test_weight_packing_launcher(host, arith, need_dx):
    import torch
    ops, _lib, rec, labels = host
    Co, Ci, k = 8, 4, 3
    w, bw = torch.zeros(Co, Ci, k), torch.zeros(1)
    wt, wd = ops._pack_weights(getattr(ops, "GEMM_" + arith), w, need_dx, bw)
    assert (wd is not None) == need_dx
    name, args = rec.calls[-1]
    assert name == _PACK[arith] and labels == [name]
    assert name in _lib.SIGNATURES and len(args) == len(_lib.SIGNATURES[name][1]) == len(_header_params(name))
    if arith == "F32":                                # fp32 layout: (Co, k*Ci) and (Ci, k*Co) floats, no size query
        assert len(rec.calls) == 1 and wt.shape == (Co, k * Ci) and wt.dtype == torch.float32
        assert wd is None or (wd.shape == (Ci, k * Co) and wd.dtype == torch.float32)
    else:                                             # plane layouts: sized by ign_clconv_x3_elems, forward then transposed form
        assert [c for c in rec.calls[:-1]] == [("ign_clconv_x3_elems", (Co, Ci, k))] + [("ign_clconv_x3_elems", (Ci, Co, k))] * need_dx
        assert wt.dtype == torch.bfloat16 and wt.numel() == 4096
    if arith == "H3":                                 # the multi-layer entry point with n = 1: one-entry host tables
        assert _header_params(name).index("w_bounds") == 8
        assert args[0] == 1 and args[7] is None and _val(args[9]) == STREAM
        tabs = [None if a is None else a[0] for a in args[1:7]] + [args[8][0]]
        assert tabs == [w.data_ptr(), wt.data_ptr(), wd.data_ptr() if need_dx else None, Co, Ci, k, bw.data_ptr()]
    else:
        assert [_val(a) for a in args] == [w.data_ptr(), wt.data_ptr(), _val(wd), Co, Ci, k, STREAM]


def test_a_linear_weight_is_packed_with_one_tap(host):
    import torch
    ops, _lib, rec, labels = host
    ops._pack_weights(ops.GEMM_X6, torch.zeros(8, 4), True)
    assert rec.calls[-1][1][3:6] == (8, 4, 1)


def test_unknown_arithmetic_is_refused_by_every_launcher(host):
    """The linear weight gradient has no fp32-MFMA form (that route is ign_clconv_wgrad with k = 1): asking for it is an error, not
    a quiet substitute."""
    ops, _lib, rec, labels = host
    ts = _tensors(9)
    with pytest.raises(KeyError):
        ops._linear_wgrad(ops.GEMM_F32, *ts[:4], 40, 4, 8)
    with pytest.raises(KeyError):
        ops._clconv_fwd("no such arithmetic", *ts[:7], DIMS)
    assert not labels
