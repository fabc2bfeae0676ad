"""Launch geometry of the row kernels, host side.  LayerNorm (csrc/ign_layernorm.hip: ln_geometry) and the instance-norm trio
(ign_instnorm_fwd / _bwd in csrc/ign_instnorm.hip, ign_instnorm_fwd_len in csrc/ign_shapelet_mask.hip) choose lanes per row,
row groups per wave, block counts, the channel tile and the block size from the problem size.  This file

  * restates both rules in Python (ln_geometry, instnorm_tile) and holds the shape tables of tests/test_gpu_launch_geometry.py
    (LN_SHAPES, LN_FWD_ONLY_SHAPES, INSTNORM_SHAPES; no torch at module level, both files import the same tables);
  * checks the LayerNorm restatement against the built library (ign_layernorm_parts: with R fixed the block count determines the
    row groups per wave), and that every table row reaches the branch it is there for -- a retuned constant fails here instead
    of letting the GPU table quietly stop crossing its branches;
  * pins the width contract: the forward takes D <= 4096, the backward refuses D > 2048 (IGN_E_TOOBIG) before any launch;
  * restates the kernels' float32 summation orders on the CPU (ln_param_grads_f32, instnorm_fwd_f32) and shows, with a defect
    planted in the RESTATEMENT (never in the library), that the comparisons of the GPU tests fail on it.

Needs no GPU.  The distances of the restatements to float64 are printed by tests/diag_launch_geometry.py."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_TOOBIG = -1001, -1003

# ------------------------------------------------------------------------------------------------------------ LayerNorm rule
LN_MAXV, LN_ITERS_MAX, LN_BLOCKS_AIM, LNR_SL = 16, 32, 2048, 16


def ln_geometry(R, D):
    """ln_geometry + what follows from it in the kernels: lanes per row G, float4 pieces per lane nv and the compiled variant NV
    that serves it, rows per wave, row groups per wave (iters), blocks, blocks per slice of layernorm_reduce_kernel, and how
    the LAST block is filled: its rows, whether a row group is cut by the `ok` predicate, whether a wave leaves its loop
    between two iterations (holds at least one but fewer than `iters` row groups)."""
    assert R > 0 and D > 0 and D % 4 == 0 and D <= 64 * 4 * LN_MAXV
    G = 1
    while G < 64 and G < D // 4:
        G <<= 1
    nv = (D // 4 + G - 1) // G
    NV = next(v for v in (1, 2, 4, 8, 16) if nv <= v)
    rpw = 64 // G
    groups = (R + rpw - 1) // rpw
    iters = min(LN_ITERS_MAX, max(1, groups // (4 * LN_BLOCKS_AIM)))
    rows_per_block = 4 * iters * rpw
    nblk = (R + rows_per_block - 1) // rows_per_block
    per = (nblk + LNR_SL - 1) // LNR_SL
    last = R - (nblk - 1) * rows_per_block
    wave_rows = [min(max(last - w * iters * rpw, 0), iters * rpw) for w in range(4)]
    wave_groups = [(r + rpw - 1) // rpw for r in wave_rows]
    return dict(G=G, nv=nv, NV=NV, rpw=rpw, iters=iters, nblk=nblk, per=per, last=last,
                cut_group=any(r % rpw for r in wave_rows), wave_breaks=any(0 < g < iters for g in wave_groups),
                reduce_batches=per // 8, reduce_tail=per % 8)


# (R, D) -> what the shape is in the table for; every entry is asserted from the restatement below
LN_SHAPES = {
    (600, 512): dict(iters=1, nblk=150, per=10, reduce_batches=1, reduce_tail=2),
    (523, 768): dict(iters=1, nv=3, NV=4, nblk=131, reduce_batches=1),
    (523, 1024): dict(iters=1, nv=4, NV=4),
    (65545, 64): dict(iters=2, rpw=4, last=9, cut_group=True),
    (262221, 16): dict(iters=2, rpw=16, last=77, cut_group=True),
    (16387, 512): dict(iters=2, rpw=1, last=3, wave_breaks=True),
    (24577, 512): dict(iters=3, rpw=1),
    (4195317, 16): dict(iters=32, rpw=16, nblk=2049, last=1013, cut_group=True),
}
LN_CAP_SHAPE = (4195317, 16)                  # 268 MB per fp32 tensor: inputs and float64 reference stay on the device
LN_RESIDUAL_SHAPES = [(65545, 64), (16387, 512)]
LN_AMAX_SHAPE = (65545, 64)
LN_FWD_ONLY_SHAPES = {(50, 2052): dict(nv=9, NV=16), (50, 4096): dict(nv=16, NV=16)}      # wider than the backward takes

# ------------------------------------------------------------------------------------------------------------ instance-norm rule
INSTNORM_LDS_AIM, INSTNORM_LDS_MAX, INSTNORM_T_MAX_TESTED = 150 * 1024, 160 * 1024, 19200


def instnorm_tile(T, C):
    """the tile rule shared by ign_instnorm_fwd, ign_instnorm_bwd and ign_instnorm_fwd_len -> channel tile CT, bytes of LDS,
    threads per block, channels of every tile of a sample"""
    CT = 32
    while CT > 1 and T * (CT + 1) * 4 > INSTNORM_LDS_AIM:
        CT >>= 1
    lds = T * (CT + 1) * 4
    return dict(CT=CT, lds=lds, threads=1024 if lds > 64 * 1024 else 256, tiles=[min(CT, C - c0) for c0 in range(0, C, CT)])


# (B, T, C) -> the tile geometry it is in the table for
INSTNORM_SHAPES = {
    (2, 496, 37): dict(CT=32, threads=256, tiles=[32, 5]),
    (2, 497, 37): dict(CT=32, threads=1024, tiles=[32, 5]),
    (2, 1163, 37): dict(CT=32, tiles=[32, 5]),
    (2, 1164, 37): dict(CT=16, tiles=[16, 16, 5]),
    (2, 2258, 37): dict(CT=16, tiles=[16, 16, 5]),
    (2, 2259, 37): dict(CT=8, tiles=[8, 8, 8, 8, 5]),
    (2, 4266, 37): dict(CT=8, tiles=[8, 8, 8, 8, 5]),
    (2, 4267, 7): dict(CT=4, tiles=[4, 3]),
    (2, 7680, 7): dict(CT=4, tiles=[4, 3]),
    (2, 7681, 7): dict(CT=2, tiles=[2, 2, 2, 1]),
    (2, 12800, 7): dict(CT=2, tiles=[2, 2, 2, 1]),
    (2, 12801, 3): dict(CT=1, tiles=[1, 1, 1]),
    (1, 17984, 6): dict(CT=1, tiles=[1] * 6),                       # EigenWorms
}
XN_TOL, GX_TOL = 1e-5, 1e-5                  # instance norm: forward element-wise, backward relative to the gradient's maximum
LN_TOL = dict(y=2e-6, gx=5e-6, dgamma=1e-5, dbeta=1e-5)             # those of test_layer_norm_against_float64


def _lib_or_skip():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("shape", list(LN_SHAPES) + list(LN_FWD_ONLY_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_layernorm_shapes_reach_their_branches(shape):
    geo = ln_geometry(*shape)
    claim = {**LN_SHAPES, **LN_FWD_ONLY_SHAPES}[shape]
    assert {k: geo[k] for k in claim} == claim, geo


def test_layernorm_table_covers_every_branch():
    geos = {s: ln_geometry(*s) for s in LN_SHAPES}
    assert {g["iters"] for g in geos.values()} >= {1, 2, 3, LN_ITERS_MAX}
    assert {g["rpw"] for g in geos.values() if g["iters"] > 1} == {1, 4, 16}
    assert any(g["cut_group"] for g in geos.values()) and any(g["wave_breaks"] for g in geos.values())
    assert any(g["reduce_batches"] and g["reduce_tail"] for g in geos.values())
    assert {g["NV"] for g in geos.values()} | {ln_geometry(*s)["NV"] for s in LN_FWD_ONLY_SHAPES} >= {1, 2, 4, 16}
    # the exact d(beta) check needs column sums of integers in -2..2 below 2^24
    assert all(2 * R < 2 ** 24 for R, _ in LN_SHAPES)
    # the cap needs 32 * 8192 wave-iterations: at 16 rows per wave (the most) one row group fewer is still `iters` = 31
    R, D = LN_CAP_SHAPE
    assert geos[LN_CAP_SHAPE]["iters"] == LN_ITERS_MAX and ln_geometry(16 * (4 * LN_BLOCKS_AIM * LN_ITERS_MAX - 1), D)["iters"] == LN_ITERS_MAX - 1
    assert set(LN_RESIDUAL_SHAPES) <= set(LN_SHAPES) and LN_AMAX_SHAPE in LN_SHAPES


@pytest.mark.parametrize("shape", list(LN_SHAPES) + list(LN_FWD_ONLY_SHAPES) + [(8, 2052), (1, 4), (256000, 512), (3904000, 64), (25600, 512)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_layernorm_restatement_agrees_with_the_library(shape):
    L = _lib_or_skip()
    assert L.ign_layernorm_parts(*shape) == ln_geometry(*shape)["nblk"]


def test_layernorm_restatement_gives_the_training_geometries():
    """Transformer benchmark, PatchTST and the EEG-CNN encoder: the geometries the table is there to reach"""
    assert [ln_geometry(*s)["iters"] for s in ((256000, 512), (3904000, 64), (25600, 512))] == [31, 32, 3]


@pytest.mark.parametrize("shape", list(INSTNORM_SHAPES), ids=lambda s: "B{}-T{}-C{}".format(*s))
def test_instnorm_shapes_reach_their_tiles(shape):
    _, T, C = shape
    tile = instnorm_tile(T, C)
    claim = INSTNORM_SHAPES[shape]
    assert {k: tile[k] for k in claim} == claim, tile
    # nothing in the table asks for more LDS than the rule aims for: the band up to the refusal at 160 KB stays untested
    assert T <= INSTNORM_T_MAX_TESTED and tile["lds"] <= INSTNORM_LDS_AIM
    assert len(tile["tiles"]) > 1                                                  # several tiles per sample ...
    if tile["CT"] > 1:
        assert tile["tiles"][-1] < tile["CT"]                                      # ... and a ragged last one


def test_instnorm_table_straddles_every_threshold():
    by_T = {T: instnorm_tile(T, C) for _, T, C in INSTNORM_SHAPES}
    assert {t["CT"] for t in by_T.values()} == {32, 16, 8, 4, 2, 1}
    for T in by_T:
        if T + 1 in by_T:
            a, b = by_T[T], by_T[T + 1]
            assert (a["CT"], a["threads"]) != (b["CT"], b["threads"]), T
    assert sum(T + 1 in by_T for T in by_T) == 6                # 256 -> 1024 threads and the five halvings of the tile
    assert instnorm_tile(INSTNORM_T_MAX_TESTED, 1)["lds"] == INSTNORM_LDS_AIM and instnorm_tile(INSTNORM_T_MAX_TESTED + 1, 1)["lds"] > INSTNORM_LDS_AIM


# ------------------------------------------------------------------------------------------------------------ width contract
def _p(v):
    return ctypes.c_void_p(v)


def test_layernorm_backward_stops_at_2048_where_the_forward_goes_to_4096():
    """D in 2052..4096: ign_layernorm_parts and ign_layernorm_fwd accept the width, ign_layernorm_bwd(_amax) returns
    IGN_E_TOOBIG (its LDS fold needs 4 * 2 * D floats) before any launch -- the pointers are dummies.  ops.layer_norm keeps
    such widths away from both (its D > 2048 guard); include/ign_abi.h states the limit."""
    L = _lib_or_skip()
    assert L.ign_layernorm_parts(8, 2052) > 0 and L.ign_layernorm_parts(8, 4096) > 0
    assert L.ign_layernorm_parts(8, 4100) == 0 and L.ign_layernorm_parts(8, 2050) == 0
    pp = _p(16)
    for D in (2052, 4096):
        assert L.ign_layernorm_bwd(pp, pp, pp, pp, pp, pp, pp, pp, pp, 8, D, None) == E_TOOBIG
        assert b"ign_layernorm_bwd:" in L.ign_last_error() and b"bytes of LDS" in L.ign_last_error()
        assert L.ign_layernorm_bwd_amax(pp, pp, pp, pp, pp, pp, pp, pp, pp, pp, 8, D, None) == E_TOOBIG
        assert b"ign_layernorm_bwd_amax:" in L.ign_last_error()
    assert L.ign_layernorm_bwd(pp, pp, pp, pp, pp, pp, pp, pp, pp, 8, 4100, None) == E_ARG
    assert L.ign_layernorm_fwd(pp, pp, pp, pp, pp, pp, 8, 4100, 1e-5, None) == E_ARG
    hdr = open(os.path.join(ROOT, "include", "ign_abi.h")).read()
    assert "D <= 4096 (backward: D <= 2048)" in hdr
    src = open(os.path.join(ROOT, "speech-imagery-eeg_amd", "ign_hip", "ops.py")).read()
    assert "D > 2048" in src[src.index("def layer_norm("):]


# ------------------------------------------------------------------------------------------------------------ float32 restatements
F32 = np.float32


def _fma32(a, b, c):
    """fp32 fma(a, b, c) through float64: the product of two floats is exact there, the sum is rounded twice (2^-53, then 2^-24)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _butterfly(v):
    """the xor-shuffle reduction over the last axis (a power of two): every lane ends with the same pairwise tree"""
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


def ln_stats_f32(x, geo):
    """mean and rstd of every row in layernorm_fwd_kernel's order: a lane's float4 pieces as (x + y) + (z + w), its pieces in
    ascending order, the xor butterfly over the G lanes of the row, times fl(1 / D); two passes.  x (R, D) float32."""
    R, D = x.shape
    G, nv = geo["G"], geo["nv"]
    xp = np.zeros((R, nv * G * 4), F32)
    xp[:, :D] = x
    xp = xp.reshape(R, nv, G, 4)
    live = (np.arange(nv * G * 4) < D).reshape(1, nv, G, 4)
    invD = F32(1.0) / F32(D)
    s = np.zeros((R, G), F32)
    for v in range(nv):
        s = s + ((xp[:, v, :, 0] + xp[:, v, :, 1]) + (xp[:, v, :, 2] + xp[:, v, :, 3]))
    mean = _butterfly(s) * invD
    d = np.where(live, xp - mean[:, None, None, None], F32(0))
    d = d * d
    q = np.zeros((R, G), F32)
    for v in range(nv):
        q = q + ((d[:, v, :, 0] + d[:, v, :, 1]) + (d[:, v, :, 2] + d[:, v, :, 3]))
    rstd = (F32(1.0) / np.sqrt(_butterfly(q) * invD + F32(1e-5))).astype(F32)
    return mean, rstd


def ln_param_grads_f32(x, gy, mean, rstd, geo, defect=None):
    """d(gamma), d(beta) in the order of layernorm_bwd_kernel + layernorm_reduce_kernel: a lane accumulates its columns over
    the `iters` row groups of its wave (d(gamma) by fma), the 4 * rpw slots of a block are summed in slot order, the blocks
    of each of the 16 slices in ascending order, then the slices.  x, gy (R, D) float32.
    defect="skip last group": wave 0 of block 0 leaves its loop one row group early -- the planted error of the teeth test."""
    R, D = x.shape
    rpw, iters, nblk, per = geo["rpw"], geo["iters"], geo["nblk"], geo["per"]
    Rp = nblk * 4 * iters * rpw
    xh = np.zeros((Rp, D), F32)
    xh[:R] = (x - mean[:, None]) * rstd[:, None]
    g = np.zeros((Rp, D), F32)
    g[:R] = gy                                                      # rows past R add +0: what `ok` leaves out
    xh, g = xh.reshape(nblk, 4, iters, rpw, D), g.reshape(nblk, 4, iters, rpw, D)
    if defect == "skip last group":
        assert iters > 1
        g = g.copy()
        g[0, 0, iters - 1] = 0
    elif defect is not None:
        raise ValueError(defect)
    dg, db = np.zeros((nblk, 4, rpw, D), F32), np.zeros((nblk, 4, rpw, D), F32)
    for it in range(iters):
        dg = _fma32(g[:, :, it], xh[:, :, it], dg)
        db = db + g[:, :, it]
    out = []
    for acc in (dg, db):
        acc = acc.reshape(nblk, 4 * rpw, D)
        part = np.zeros((nblk, D), F32)
        for sl in range(4 * rpw):
            part = part + acc[:, sl]
        pp = np.zeros((LNR_SL * per, D), F32)
        pp[:nblk] = part
        pp = pp.reshape(LNR_SL, per, D)
        s = np.zeros((LNR_SL, D), F32)
        for b in range(per):
            s = s + pp[:, b]
        t = np.zeros(D, F32)
        for sl in range(LNR_SL):
            t = t + s[sl]
        out.append(t)
    return out[0], out[1]


def instnorm_fwd_f32(x, CT, defect=None, eps=1e-8):
    """xn (B, C, T) in instnorm_kernel's order: per channel, lane l sums t = l, l + 64, ... serially, the 64 lanes fold by the
    xor butterfly, mean = s / T; the centred squares the same way by fma; (x - mean) / (sqrt(v / (T - 1)) + eps).  x (B, T, C)
    float32.  Planted errors of the teeth tests: defect="one sample short": mean and std are those of the first T - 1
    samples; defect="stale tile statistics": the ragged last channel tile is normalised with the previous tile's mean and std."""
    B, T, C = x.shape
    n = (T + 63) // 64
    xc = np.zeros((B, C, n * 64), F32)
    xc[:, :, :T] = x.transpose(0, 2, 1)
    Ts = T - 1 if defect == "one sample short" else T
    live = (np.arange(n * 64) < Ts).reshape(n, 64)
    xr = xc.reshape(B, C, n, 64)
    s = np.zeros((B, C, 64), F32)
    for i in range(n):
        s = s + np.where(live[i], xr[:, :, i], F32(0))
    mean = _butterfly(s) / F32(Ts)
    v = np.zeros((B, C, 64), F32)
    for i in range(n):
        dv = np.where(live[i], xr[:, :, i] - mean[..., None], F32(0))
        v = _fma32(dv, dv, v)
    denom = np.sqrt(_butterfly(v) / F32(Ts - 1)) + F32(eps)
    if defect == "stale tile statistics":
        c0 = (C - 1) // CT * CT
        assert 0 < c0 and C - c0 < CT
        mean, denom = mean.copy(), denom.copy()
        mean[:, c0:], denom[:, c0:] = mean[:, c0 - CT:c0 - CT + C - c0], denom[:, c0 - CT:c0 - CT + C - c0]
    elif defect not in (None, "one sample short"):
        raise ValueError(defect)
    return ((xc[:, :, :T] - mean[..., None]) / denom[..., None]).astype(F32)


def instnorm_f64(x):
    """(B, T, C) -> (B, C, T) in float64: the arithmetic of oracle.ign_oracle.instance_norm on x.double(), in numpy"""
    xc = np.asarray(x, np.float64).transpose(0, 2, 1)
    return (xc - xc.mean(-1, keepdims=True)) / (xc.std(-1, ddof=1, keepdims=True) + 1e-8)


def instnorm_input(B, T, C, seed=None):
    """x = randn * 3 + 50 (the large-offset recipe of the instance-norm tests), float32 numpy; the GPU tests use the same batch"""
    rng = np.random.default_rng(T * 64 + C if seed is None else seed)
    return (rng.standard_normal((B, T, C)) * 3.0 + 50.0).astype(F32)


def _must_fail(label, got, ref, **kw):
    """the comparison of the GPU tests (conftest.parity) must REFUSE `got`; the record it made is taken out of the ledger again,
    which is the list of errors observed on the device"""
    import conftest
    with pytest.raises(AssertionError):
        conftest.parity(label, got, ref, **kw)
    for recs in conftest._LEDGER.values():
        recs.pop(label, None)
    for k in [k for k, v in conftest._LEDGER.items() if not v]:
        del conftest._LEDGER[k]


def _must_pass(label, got, ref, **kw):
    import conftest
    conftest.parity(label, got, ref, **kw)
    for recs in conftest._LEDGER.values():
        recs.pop(label, None)
    for k in [k for k, v in conftest._LEDGER.items() if not v]:
        del conftest._LEDGER[k]


def test_instnorm_oracle_restatement_is_the_oracle():
    import torch
    from oracle import ign_oracle as O
    x = instnorm_input(2, 497, 5)
    np.testing.assert_array_equal(instnorm_f64(x).shape, (2, 5, 497))
    np.testing.assert_allclose(instnorm_f64(x), O.instance_norm(torch.from_numpy(x).double()).numpy(), rtol=1e-12, atol=1e-12)


def test_teeth_a_skipped_row_group_changes_the_integer_column_sums():
    """Section 1's row-coverage check on the CPU: with gy integer in -2..2 the float32 restatement of the backward's summation
    order gives the column sums exactly (any order does); with one row group of one wave skipped it does not -- at a shape
    whose d(beta) of random gradients would also have to be told apart through a tolerance."""
    R, D = 16387, 512
    geo = ln_geometry(R, D)
    assert geo["iters"] == 2
    rng = np.random.default_rng(5)
    gy = rng.integers(-2, 3, size=(R, D)).astype(F32)
    x = rng.standard_normal((R, D)).astype(F32)
    zero, one = np.zeros(R, F32), np.ones(R, F32)
    exact = gy.astype(np.int64).sum(0)
    _, db = ln_param_grads_f32(x, gy, zero, one, geo)
    _must_pass("restated d(beta), integer gy", db, exact, tol=0.0, kind="scale")
    _, db = ln_param_grads_f32(x, gy, zero, one, geo, defect="skip last group")
    assert 0 < np.count_nonzero(db != exact)
    _must_fail("planted: row group skipped, d(beta)", db, exact, tol=0.0, kind="scale")


def test_teeth_one_sample_missing_from_the_statistics_at_eigenworms_length():
    """Section 2's forward comparison (1e-5 element-wise against float64) on the CPU, T = 17 984: the float32 restatement of the
    kernel's order passes it, the same restatement with the last sample left out of both sums fails it -- and would have
    passed the 1e-4 of the older instance-norm tests only just."""
    B, T, C = 1, 17984, 6
    x = instnorm_input(B, T, C)
    ref = instnorm_f64(x)
    CT = instnorm_tile(T, C)["CT"]
    _must_pass("restated xn", instnorm_fwd_f32(x, CT), ref, tol=XN_TOL, kind="elem")
    bad = instnorm_fwd_f32(x, CT, defect="one sample short")
    _must_fail("planted: one sample short, xn", bad, ref, tol=XN_TOL, kind="elem")
    worst = float((np.abs(bad - ref) / (1 + np.abs(ref))).max())
    assert 5 * XN_TOL < worst < 5e-4, worst


@pytest.mark.parametrize("shape", [(2, 1164, 37), (2, 4267, 7), (2, 7681, 7)], ids=lambda s: "B{}-T{}-C{}".format(*s))
def test_teeth_stale_statistics_in_the_ragged_last_tile(shape):
    """the ragged last channel tile normalised with the previous tile's statistics: every channel of the recipe has mean ~50 and
    std ~3, so the outputs still look normalised -- the 1e-5 comparison refuses them, and only in the last tile's channels"""
    B, T, C = shape
    x = instnorm_input(B, T, C)
    ref = instnorm_f64(x)
    CT = instnorm_tile(T, C)["CT"]
    good, bad = instnorm_fwd_f32(x, CT), instnorm_fwd_f32(x, CT, defect="stale tile statistics")
    _must_pass("restated xn", good, ref, tol=XN_TOL, kind="elem")
    _must_fail("planted: stale tile statistics, xn", bad, ref, tol=XN_TOL, kind="elem")
    c0 = (C - 1) // CT * CT
    np.testing.assert_array_equal(bad[:, :c0], good[:, :c0])
