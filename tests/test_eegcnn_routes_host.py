"""EEG-CNN off its fast window, host side.  tests/eegcnn_route_cases.py restates the dispatch rules of csrc/ign_eegcnn.hip
(xcorr_geometry, the T <= 1024 switch of ign_dwconv1d_fwd / ign_autocorr_fwd), csrc/ign_eegcnn_fused.hip (cw_blocks, the MFMA /
VALU choice of ign_chan_contract_bwd_weight) and models/eegcnn.py (the BatchNorm-1 routes) and holds the shape tables of
tests/test_gpu_eegcnn_routes.py.  This file

  * proves from the restatement that every table row reaches the route it is there for -- a retuned constant fails here instead
    of quietly emptying a GPU case -- and that the tables cover every route;
  * confirms the restatement from the built library where that needs no device (workspace sizes give block counts; the refusals
    of ign_autocorr_sum_fwd come before any launch);
  * checks EEGcnn._shifted_sums, which is plain torch, against the brute-force per-tap sums of the zero-padded rows in float64,
    rows shorter than the left pad included;
  * states the refusal rule for kernels beyond 128 taps once.

Needs no GPU.  The GPU distances are recorded by tests/diag_eegcnn_routes.py."""
import ctypes
import os

import numpy as np
import pytest

import eegcnn_route_cases as R


def _lib_or_skip():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    return _lib.lib()


def _has(got, want, row):
    for key, v in want.items():
        assert got[key] == v, f"{row}: {key} = {got[key]!r}, the row is there for {v!r}"


# ---------------------------------------------------------------------------------------------------- rows reach their routes
@pytest.mark.parametrize("shape,want,why", R.DWCONV_CASES, ids=[str(c[0]) for c in R.DWCONV_CASES])
def test_dwconv_rows_reach_their_kernels(shape, want, why):
    B, C, T, k = shape
    got = R.dwconv_route(T, k, B)
    assert got["refused"] == 0, (shape, why)
    _has(got, want, (shape, why))


def test_dwconv_table_covers_every_branch():
    routes = [R.dwconv_route(T, k, B) for (B, C, T, k), _, _ in R.DWCONV_CASES]
    wave = [r for r in routes if r["fwd"] == "dwconv1d_wave_kernel"]
    assert {r["TT"] for r in wave} == {4, 8, 16}
    assert {r["TT"] for r in wave if r["full_lanes"]} == {4, 8, 16}                 # T = 256, 512, 1024: no idle lane
    assert any(r["tap_groups"] == 0 and r["TT"] in (8, 16) for r in wave)           # tail-only tap loop at a wide lane tile
    assert any(r["tap_groups"] and r["tap_tail"] for r in wave) and any(r["tap_groups"] and not r["tap_tail"] for r in wave)
    generic = [r for r in routes if r["fwd"] == "dwconv1d_kernel"]
    assert {r["t_mod4"] for r in generic} == {0, 1, 2, 3}
    fallback = [r for r in routes if r["dw"] == "dwconv1d_bwd_w_kernel"]
    assert any(r["fwd"] == "dwconv1d_wave_kernel" for r in fallback) and any(r["fwd"] == "dwconv1d_kernel" for r in fallback)
    assert any(r["tap_slots"] > 1 for r in fallback) and any(len(r["rows_per_slab"]) > 1 for r in fallback)
    assert any(k % 2 == 0 for (_, _, _, k), _, _ in R.DWCONV_CASES)
    # the switch points themselves
    assert R.dwconv_route(1024, 25)["fwd"] == "dwconv1d_wave_kernel" and R.dwconv_route(1025, 25)["fwd"] == "dwconv1d_kernel"
    assert R.dwconv_route(1024, 128)["dw"] == "xcorr_kernel" and R.dwconv_route(1024, 129)["dw"] == "dwconv1d_bwd_w_kernel"
    assert R.dwconv_route(1025, 128)["dw"] == "dwconv1d_bwd_w_kernel"
    assert R.dwconv_route(8000, 184)["refused"] == 0 and R.dwconv_route(8000, 185)["refused"] == R.E_TOOBIG


@pytest.mark.parametrize("shape,want,why", R.AUTOCORR_CASES, ids=[str(c[0]) for c in R.AUTOCORR_CASES])
def test_autocorr_rows_reach_their_kernels(shape, want, why):
    Rr, T, K = shape
    got = R.autocorr_route(T, K, Rr)
    assert got["refused"] == 0
    _has(got, want, (shape, why))


@pytest.mark.parametrize("shape,want,why", R.GRAM_CASES, ids=[str(c[0]) for c in R.GRAM_CASES])
def test_gram_rows_reach_their_routes(shape, want, why):
    Rr, T, k, pl = shape
    assert pl == (k - 1) // 2 and T >= k
    assert R.autocorr_route(T, k, Rr)["kernel"] == want["kernel"] and R.gram_edges(k) == want["edges"], (shape, why)
    assert R.gram_edges(125) == "edge_lagprod" and R.gram_edges(126) == "torch"


@pytest.mark.parametrize("shape,why", R.SUMSQ_CASES, ids=[str(c[0]) for c in R.SUMSQ_CASES])
def test_conv1_sumsq_rows_are_shapes_the_model_routes_there(shape, why):
    Rr, T, F1, k1 = shape
    assert (T > 1024) + (T < k1) + (k1 > 128) >= 1, (shape, why)          # outside what the fast-window tests cover
    assert not R.conv1_sumsq_bwd_refuses(F1, k1)
    assert R.bn1_route(T, k1, F1, variance_switch="conv") == "conv"
    if T < k1 or k1 > 128:
        assert R.bn1_route(T, k1, F1) == "conv"                           # ... also without the switch


@pytest.mark.parametrize("shape,off,want,why", R.CHAN_CASES, ids=[f"{c[0]}+{c[1]}" for c in R.CHAN_CASES])
def test_chan_contract_rows_reach_their_plan(shape, off, want, why):
    B, Ci, Co, T = shape
    _has(R.cw_plan(B, T, aligned=off % 4 == 0), want, (shape, why))
    assert Ci <= 128 and Co <= 64


@pytest.mark.parametrize("case", R.MODEL_CASES, ids=[c[0] for c in R.MODEL_CASES])
def test_model_rows_reach_their_bn1_route(case):
    name, shape, opts, route, why = case
    B, C, T, k1, k2, F1, D, P1, P2 = shape
    assert R.model_kernels(shape, opts)["bn1"] == route, (name, why)
    assert C <= 128 and F1 * D <= 64 and (T // P1) // P2 >= 1


def test_model_table_covers_every_route_and_kernel():
    ks = {name: R.model_kernels(shape, opts) for name, shape, opts, _, _ in R.MODEL_CASES}
    assert {k["bn1"] for k in ks.values()} == {"fold", "gram/edge_lagprod", "gram/torch", "conv"}
    assert ks["long"]["lag_sums"] == "autocorr_kernel" and ks["k127"]["lag_sums"] == "xcorr_kernel"
    assert ks["long"]["block1"]["fwd"] == "dwconv1d_kernel" and ks["long"]["block1"]["dw"] == "dwconv1d_bwd_w_kernel"
    assert ks["long"]["block2"]["fwd"] == "dwconv1d_wave_kernel"
    assert ks["T1024"]["block1"]["fwd"] == "dwconv1d_wave_kernel" and ks["T1025"]["block1"]["fwd"] == "dwconv1d_kernel"
    assert ks["k131"]["block1"]["dw"] == "dwconv1d_bwd_w_kernel" and ks["k131"]["block1"]["fwd"] == "dwconv1d_wave_kernel"
    # the two rows that differ from a fast-window row only by a switch
    assert R.bn1_route(200, 31, 4) == "fold"
    assert R.bn1_route(200, 31, 4, momentum=None, track=False) == "fold"
    # the refusals
    for spec in (R.REFUSED_TAPS, R.REFUSED_ROW):
        B, C, T, k1, k2, F1, D, P1, P2 = spec["shape"]
        assert R.bn1_route(T, k1, F1) == "refused", spec
    B, C, T, k1, k2, F1, D, P1, P2 = R.REFUSED_TAPS["shape"]
    assert R.bn1_route(T, k1, F1, needs_grad=False) == "conv"             # the forward alone runs: only the gradient is missing
    B, C, T, k1, k2, F1, D, P1, P2 = R.REFUSED_ROW["shape"]
    assert R.dw_check(T, k1) == R.E_TOOBIG and R.autocorr_route(T, k1)["refused"] == R.E_TOOBIG


# ---------------------------------------------------------------------------------------------------- the refusal rule, once
def test_refusal_rule_beyond_128_taps():
    """ign_conv1_sumsq_bwd holds one lane per (filter, four taps) of at most eight filters in a block of 256:
    ceil(k1 / 4) * min(F1, 8) <= 256, i.e. k1 <= 4 * (256 // min(F1, 8)).  The lag-sum route needs no such pass but ends at 128
    taps, so beyond 128 taps the default F1 = 8 cannot train at all and the model says so from forward."""
    assert [R.conv1_sumsq_max_taps(F1) for F1 in (2, 4, 8)] == [512, 256, 128]
    for F1 in (1, 2, 3, 4, 7, 8, 9, 16):
        kmax = R.conv1_sumsq_max_taps(F1)
        assert not R.conv1_sumsq_bwd_refuses(F1, kmax) and R.conv1_sumsq_bwd_refuses(F1, kmax + 1), F1
    import speech_imagery_eeg_amd  # noqa: F401
    from models import eegcnn
    assert [eegcnn.conv1_sumsq_max_taps(F1) for F1 in (1, 2, 3, 4, 7, 8, 9, 16)] == \
        [R.conv1_sumsq_max_taps(F1) for F1 in (1, 2, 3, 4, 7, 8, 9, 16)]
    assert eegcnn._ROW_TILE_MAX == R.ROW_TILE_MAX
    assert R.dw_check(R.ROW_TILE_MAX - 25, 25) == 0 and R.dw_check(R.ROW_TILE_MAX - 24, 25) == R.E_TOOBIG
    assert eegcnn._BN1_VARIANCE == "gram"
    for k1 in (129, 131, 200):
        assert R.bn1_route(200, k1, 8) == "refused" and R.bn1_route(200, k1, 4) == "conv"
    assert R.bn1_route(40, 65, 8) == "conv" and R.bn1_route(40, 128, 8) == "conv" and R.bn1_route(40, 129, 8) == "refused"


# ---------------------------------------------------------------------------------------------------- the library, no device
@pytest.mark.parametrize("shape,off,want,why", R.CHAN_CASES, ids=[f"{c[0]}+{c[1]}" for c in R.CHAN_CASES])
def test_chan_contract_block_count_agrees_with_the_library(shape, off, want, why):
    L = _lib_or_skip()
    B, Ci, Co, T = shape
    assert L.ign_chan_contract_bwd_weight_workspace_bytes(B, Ci, Co, T) == want["blocks"] * Co * Ci * 4
    for b, t in ((1, 1), (7, 64), (8, 64 * 64), (8, 64 * 64 + 1), (511, 64), (513, 60)):
        assert L.ign_chan_contract_bwd_weight_workspace_bytes(b, Ci, Co, t) == R.cw_plan(b, t)["blocks"] * Co * Ci * 4, (b, t)


def test_partial_buffer_sizes_agree_with_the_library():
    L = _lib_or_skip()
    for (Rr, T, K), _, _ in R.AUTOCORR_CASES:
        parts = L.ign_autocorr_parts(Rr)
        assert parts == 2 * ((Rr + R.AC_ROWS - 1) // R.AC_ROWS)
        assert parts >= R.autocorr_route(T, K, Rr)["blocks"] * (2 if T > 1024 else 1)
    for (B, C, T, k), _, _ in R.DWCONV_CASES:
        assert L.ign_dwconv1d_bwd_weight_workspace_bytes(B, C, k) >= R.dwconv_route(T, k, B)["slabs"] * C * k * 4, (B, C, T, k)


def test_autocorr_sum_refusals_agree_with_the_library():
    """where the restatement says xcorr_geometry refuses, ign_autocorr_sum_fwd returns IGN_E_UNSUP before it touches its
    buffers or the device (shapes it accepts are asked on the GPU: tests/test_gpu_eegcnn_routes.py)"""
    L = _lib_or_skip()
    buf = (ctypes.c_float * 4096)()
    used = ctypes.c_int(0)
    p = ctypes.cast(buf, ctypes.c_void_p)
    shapes = {(T, k) for (_, _, T, k), _, _ in R.DWCONV_CASES} | {(T, K) for (_, T, K), _, _ in R.AUTOCORR_CASES} | \
        {(T, k) for (_, T, k, _), _, _ in R.GRAM_CASES} | {(1025, 1), (1024, 129), (4000, 128)}
    refused = [s for s in sorted(shapes) if s[1] <= R.AC_LAGS and R.autocorr_sum_refuses(*s)]
    assert len(refused) >= 8
    for T, K in refused:
        assert L.ign_autocorr_sum_fwd(p, p, p, 1, T, K, ctypes.byref(used), None) == R.E_UNSUP, (T, K)
    assert all(T > 1024 for T, _ in refused)          # for K <= 128 the geometry refuses nothing but long rows
    for T in (1, 2, 5, 63, 64, 65, 128, 129, 233, 256, 257, 1000, 1021, 1024):
        for K in (1, 32, 33, 128):
            g = R.xcorr_geometry(T, K)
            assert g is not None and g["lds"] <= R.LDS_64K and g["rpp"] * g["T4"] <= 256 * R.XC_NA, (T, K)


# ---------------------------------------------------------------------------------------------------- _shifted_sums
@pytest.mark.parametrize("T,k", R.SHIFTED_SUMS_CASES)
def test_shifted_sums_equal_brute_force(T, k):
    """S[j] = sum over samples, electrodes and output positions of the zero-padded row at tap j ('same' padding (k-1)//2 on the
    left): the data side of BatchNorm-1's batch mean, at any T >= 1."""
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from models.eegcnn import EEGcnn
    pl = (k - 1) // 2
    g = torch.Generator().manual_seed(1000 * T + k)
    x = torch.randn(3, 4, T, generator=g, dtype=torch.float64) * 1.5 + 0.2
    S = EEGcnn._shifted_sums(x, k, pl)
    xp = np.pad(x.numpy(), ((0, 0), (0, 0), (pl, k - 1 - pl)))
    ref = np.array([xp[..., j:j + T].sum() for j in range(k)])
    assert tuple(S.shape) == (k,), f"T={T} k={k}: {tuple(S.shape)} entries for {k} taps"
    err = float(np.abs(S.numpy() - ref).max()) / float(np.abs(ref).max())
    print(f"_shifted_sums T={T} k={k}: max error {err:.2e} of the largest sum")
    assert err <= R.SHIFTED_SUMS_TOL
    if T < pl:
        assert S[0] == 0 and S[-1] == 0                 # taps further than T from the centre see no sample
