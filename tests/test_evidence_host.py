"""Evidence maps on the host (no GPU): the three entry points are declared, bound and exported and refuse bad arguments before any
launch; the numpy restatement (utils/evidence.py restates csrc/ign_evidence.h) against a direct triple loop written in
tests/evidence_cases.py; completeness of the rule; t = -1; the edge arithmetic of the spread; the --evidence flag.  The GPU side is
tests/test_gpu_evidence.py.

Bounds (none is measured).  v = fl(fl(W p) fl(1/L)) differs from W p / L by at most 2 roundings beyond the product's, an output
element adds at most sum K such terms (sum K - 1 roundings) and is scaled once: |sum_{s,c} E - sum_f W p| <= (sum K + 3) 2^-24
sum_f |W p|.  E_dnn[s] = fl(fl(1/R) acc) with acc a sum of at most R terms, every cam[t] in R windows:
|sum_s E_dnn - sum_t cam| <= (R + 3) 2^-24 sum_t |cam|."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from evidence_cases import BANK, CLASSES, SHAPES, U, cam_spread_loop, evidence_loop, make_case, same_bits

import speech_imagery_eeg_amd  # noqa: F401
from utils import evidence as E

BANKF, CAM, SPREAD = "ign_shapelet_evidence_bank", "ign_bn_relu_cam_fwd", "ign_cam_spread"
E_ARG, E_TOOBIG = -1001, -1003


def _lib_or_skip():
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    return _lib


def _header_params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
    assert m, name
    return [re.split(r"[\s*]+", p.strip())[-1] for p in m.group(1).split(",")]


# ---------------------------------------------------------------- ABI
def test_new_symbols_are_declared_bound_and_exported():
    from ign_hip import _lib, ops
    assert _header_params(BANKF) == ["p", "t", "W", "target", "scale", "ld", "G", "K", "L", "stride", "col0", "invL", "out", "B", "T",
                                     "C", "N", "stream"]
    assert _header_params(CAM) == ["y_last", "a", "b", "head_w", "target", "scale", "cam", "B", "Tl", "Cl", "N", "stream"]
    assert _header_params(SPREAD) == ["cam", "out", "B", "Tl", "R", "invR", "stream"]
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.SIGNATURES[BANKF] == (ci, [vp] * 5 + [ci, ci] + [vp] * 6 + [ci] * 4 + [vp])
    assert _lib.SIGNATURES[CAM] == (ci, [vp] * 7 + [ci] * 4 + [vp])
    assert _lib.SIGNATURES[SPREAD] == (ci, [vp, vp, ci, ci, ci, cf, vp])
    assert all(callable(getattr(ops, f)) for f in ("shapelet_evidence", "fcn_cam", "cam_spread"))
    rule = open(os.path.join(ROOT, "speech-imagery-eeg_amd", "csrc", "ign_evidence.h")).read()
    assert not re.search(r"\bfmaf?\s*\(", re.sub(r"//[^\n]*", "", rule))            # one rounding per operation, restatable
    _lib_or_skip()
    h = ctypes.CDLL(_lib.lib_path())
    assert hasattr(h, BANKF) and hasattr(h, CAM) and hasattr(h, SPREAD)


def test_entry_points_refuse_bad_arguments_without_a_device():
    """every refusal returns before a launch: the pointers are not device memory and no GPU is needed to run this"""
    h = _lib_or_skip().lib()
    q = ctypes.c_void_p(1 << 20)
    ints, floats = ctypes.c_int * 2, ctypes.c_float * 2

    def bank(ld=50, G=2, K=(2, 3), L=(4, 19), stride=(1, 2), col0=(0, 10), B=3, T=37, C=5, N=3, p=q, out=q):
        return h.ign_shapelet_evidence_bank(p, q, q, q, None, ld, G, ints(*K), ints(*L), ints(*stride), ints(*col0),
                                            floats(0.25, 1 / 19), out, B, T, C, N, None)

    assert bank(ld=49) == E_ARG and b"ld=49" in h.ign_last_error()
    assert bank(col0=(0, 15)) == E_ARG
    assert bank(G=0) == E_ARG and bank(G=9) == E_ARG
    assert bank(L=(4, 38)) == E_ARG and bank(L=(0, 19)) == E_ARG and bank(stride=(1, 0)) == E_ARG and bank(K=(0, 3)) == E_ARG
    assert bank(p=None) == E_ARG and bank(out=None) == E_ARG and bank(B=0) == E_ARG and bank(N=0) == E_ARG
    assert bank(T=1 << 22, C=1 << 10, ld=5 << 10, col0=(0, 2 << 10)) == E_TOOBIG

    def cam(y=q, B=2, Tl=5, Cl=128, N=3):
        return h.ign_bn_relu_cam_fwd(y, q, q, q, q, None, q, B, Tl, Cl, N, None)

    assert cam(Cl=6) == E_ARG and cam(Cl=0) == E_ARG and cam(Cl=1028) == E_ARG and cam(Tl=0) == E_ARG and cam(y=None) == E_ARG
    assert cam(y=ctypes.c_void_p((1 << 20) + 4)) == E_ARG and b"aligned" in h.ign_last_error()
    assert h.ign_cam_spread(q, q, 2, 5, 0, 1.0, None) == E_ARG and h.ign_cam_spread(q, q, 2, 0, 6, 1.0, None) == E_ARG
    assert h.ign_cam_spread(None, q, 2, 5, 6, 1.0, None) == E_ARG


# ---------------------------------------------------------------- the rule
@pytest.mark.parametrize("shape", SHAPES[:3], ids=str)
@pytest.mark.parametrize("scale", [False, True], ids=["plain", "scaled"])
def test_rule_equals_the_triple_loop(shape, scale):
    B, T, C = shape
    case = make_case(B, T, C, CLASSES[shape[2] % 2], seed=B + T + C, scale=scale, **BANK)
    got = E.evidence_rule(case["p"], case["t"], case["W"], case["target"], case["Ks"], case["Ls"], case["strides"], C, T, case["scale"])
    assert got.dtype == np.float32 and got.shape == (B, T, C)
    assert same_bits(got, evidence_loop(case))                     # the float32 rule, operation by operation
    exact = evidence_loop(case, exact=True)                          # and what it approximates: W p / L summed in float64
    n = sum(case["Ks"])
    mag = evidence_loop(dict(case, W=np.abs(case["W"])), exact=True)
    assert (np.abs(got - exact) <= (n + 3) * U * np.abs(mag) + 1e-300).all()


def test_rule_is_complete_and_skips_unmatched_features():
    B, T, C, N = 3, 37, 5, 3
    case = make_case(B, T, C, N, seed=5, **BANK)
    p, t, W, tg = case["p"], case["t"], case["W"], case["target"]
    got = E.evidence_rule(p, t, W, tg, case["Ks"], case["Ls"], case["strides"], C, T).astype(np.float64)
    contrib = (W[tg] * p).astype(np.float64) * (t >= 0)
    assert (t == -1).sum() == 2
    bound = (sum(case["Ks"]) + 3) * U * np.abs(contrib).sum(1)
    assert (np.abs(got.sum((1, 2)) - contrib.sum(1)) <= bound).all()
    # a feature with t = -1 contributes nothing: giving it any value changes no bit; giving it a window does
    f = int(np.argwhere(t[0] == -1)[0, 0])
    p2 = p.copy()
    p2[0, f] = 1e6
    again = E.evidence_rule(p2, t, W, tg, case["Ks"], case["Ls"], case["strides"], C, T)
    assert same_bits(again, got.astype(np.float32))
    t2 = t.copy()
    t2[0, f] = 0
    assert not same_bits(E.evidence_rule(p2, t2, W, tg, case["Ks"], case["Ls"], case["strides"], C, T), got.astype(np.float32))
    # positions no window covers are exactly zero
    only = np.full_like(t, -1)
    only[:, 0] = 3
    one = E.evidence_rule(p, only, W, tg, case["Ks"], case["Ls"], case["strides"], C, T)
    L0 = case["Ls"][0]
    assert (one[:, 3:3 + L0, 0] != 0).all() and np.count_nonzero(one) == B * L0


@pytest.mark.parametrize("R", [6, 14])
def test_cam_spread_rule_edges_and_completeness(R):
    rng = np.random.default_rng(R)
    for Tl in (1, 2, R - 1, R, 67):
        cam = rng.standard_normal((2, Tl)).astype(np.float32)
        got = E.cam_spread_rule(cam, R)
        assert got.shape == (2, Tl + R - 1) and got.dtype == np.float32
        assert same_bits(got, cam_spread_loop(cam, R))
        bound = (R + 3) * U * np.abs(cam.astype(np.float64)).sum(1)
        assert (np.abs(got.astype(np.float64).sum(1) - cam.astype(np.float64).sum(1)) <= bound).all()
    # Tl = 1, T = R: the one step is spread over all R input samples, each fl(fl(1/R) * cam)
    one = E.cam_spread_rule(np.array([[3.0]], np.float32), R)
    assert one.shape == (1, R) and (one == np.float32(1.0) / np.float32(R) * np.float32(3.0)).all()


# ---------------------------------------------------------------- the flag
def test_evidence_flag_parses_and_defaults_to_none():
    import run
    base = ["--model", "SBM", "--data", "SYNTH"]
    assert run.build_parser().parse_args(base).evidence == "none"
    for v in ("none", "sbm", "gated", "dnn"):
        assert run.build_parser().parse_args(base + ["--evidence", v]).evidence == v
    for bad in ("all", "SBM", ""):
        with pytest.raises(SystemExit):
            run.build_parser().parse_args(base + ["--evidence", bad])
    # default: nothing of the evidence path is touched -- run.main reaches it through write_evidence alone, behind the flag, and
    # neither run.py nor the experiment module imports utils.evidence at module level
    import inspect
    import exp.experiment_classification as X
    guard = [ln for ln in inspect.getsource(run.main).splitlines() if "EXPLAIN_FLAGS" in ln or "writer(" in ln or "_flag_on(" in ln]
    assert len(guard) == 3 and "_flag_on(args, flag)" in guard[1] and "!= 'none'" in inspect.getsource(run._flag_on)
    assert "evidence" not in inspect.getsource(run.main)
    rows = [row for row in run.EXPLAIN_FLAGS if row[0] == "evidence"]
    assert len(rows) == 1 and rows[0][1] is None and "write_evidence(" in inspect.getsource(rows[0][3])
    assert not run._flag_on(run.build_parser().parse_args(base), "evidence")
    assert not hasattr(run, "evidence_map") and not hasattr(X, "evidence_map") and not hasattr(X, "Evidence")


def test_dispatch_refusals_need_no_device():
    import torch
    from conftest import make_cfg
    from models.InterpGN import InterpGN
    from models.Shapelet import ShapeBottleneckModel
    x = torch.zeros(2, 100, 6)
    for cls in ("bilinear", "attention"):
        with pytest.raises(ValueError, match="not additive"):
            E.evidence_map(ShapeBottleneckModel(make_cfg(sbm_cls=cls)), x)
    with pytest.raises(TypeError, match="evidence_map"):
        E.evidence_map(torch.nn.Linear(2, 2), x)
    with pytest.raises(TypeError, match="FCN"):
        E.evidence_map(ShapeBottleneckModel(make_cfg()), x, explain="dnn")
    with pytest.raises(TypeError, match="FCN is the supported deep expert"):
        E.evidence_map(InterpGN(make_cfg(dnn_type="ResNet")), x, explain="gated")
    with pytest.raises(ValueError, match="explain"):
        E.evidence_map(ShapeBottleneckModel(make_cfg()), x, explain="all")
