"""LayerNorm and instance norm against float64 on BOTH sides of every rule by which their launchers size a launch
(csrc/ign_layernorm.hip: ln_geometry; csrc/ign_instnorm.hip and csrc/ign_shapelet_mask.hip: the channel-tile rule).  The shape
tables, the Python restatement of the two rules and the proof that each shape reaches its branch are in
tests/test_launch_geometry_host.py (no GPU); this file runs them.

LayerNorm: y, gx, d(gamma), d(beta) at the bounds of test_layer_norm_against_float64 (2e-6, 5e-6, 1e-5, 1e-5 of the tensor's
maximum, not widened for 4.2 M rows: the float32 restatement of the backward's summation order stays within 4.1e-7 of float64,
profiles/launch_geometry.json), bitwise repeatability, and at every shape with more than one row group per wave a second backward
with integer gy in -2..2: the column sums stay below 2^24, so d(beta) is exact in fp32 in ANY order and must equal them exactly --
a dropped or doubled row, which a tolerance on a sum of millions of terms cannot be relied on to see, changes an integer.
Instance norm: xn at 1e-5 element-wise (ten times tighter than the older tests: the restated float32 order is within 2.3e-6,
one sample missing from the statistics costs 1.1e-4 at T = 17 984 and more below), the raw transpose and the input bound exactly,
the gradient at 1e-5 of its maximum, exact zeros for a constant channel planted in the ragged last tile, and the length-aware
forward on truncated samples with garbage in the padding.

(R, D) tensors are compared on the device and handed to conftest.parity through the two elements that decide a kind="scale"
comparison (_rows_close): the ledger entry is that of the whole tensor, without 537 MB of float64 crossing to the host.
IGN_LAUNCH_GEOMETRY_OUT=<file>: the wall time of every LayerNorm case is written there as JSON (merged into
profiles/launch_geometry.json by tests/diag_launch_geometry.py --cases)."""
import ctypes
import functools
import json
import os
import time

import numpy as np
import pytest
import torch

import test_launch_geometry_host as H
from conftest import parity

pytestmark = pytest.mark.gpu
_WALL = {}
LN_IDS = [f"{R}x{D}" for R, D in H.LN_SHAPES]
IN_IDS = ["B{}-T{}-C{}".format(*s) for s in H.INSTNORM_SHAPES]


@pytest.fixture(scope="module", autouse=True)
def _write_wall_times():
    yield
    path = os.environ.get("IGN_LAUNCH_GEOMETRY_OUT")
    if _WALL and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(gpu_wall_time_s=_WALL), f, indent=1, sort_keys=True)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ops():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ops
    return ops, _lib


def _rows_close(label, got, ref, tol):
    """conftest.parity(kind="scale") of two device tensors of one shape: max |got - ref| and max |ref| are each attained at one
    element, and parity on those two elements records and judges exactly what it would on the whole tensors (a NaN wins
    torch's argmax, and fails)."""
    assert got.shape == ref.shape, f"{label}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    g, r = got.detach().reshape(-1), ref.detach().reshape(-1).to(got.device)
    i = torch.stack(((g.double() - r.double()).abs().argmax(), r.abs().argmax()))
    return parity(label, g[i], r[i], tol=tol, kind="scale")


def _layer_norm_pair(D, dev, seed):
    """-> (nn.LayerNorm on the device, gamma in [0.5, 1.5] and a bias; its float64 twin on the CPU)"""
    g = torch.Generator().manual_seed(seed)
    ln = torch.nn.LayerNorm(D)
    with torch.no_grad():
        ln.weight.copy_(torch.rand(D, generator=g) + 0.5)
        ln.bias.copy_(torch.randn(D, generator=g) * 0.3)
    ref = torch.nn.LayerNorm(D).double()
    ref.load_state_dict({k: v.double() for k, v in ln.state_dict().items()})
    return ln.to(dev), ref


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("shape", list(H.LN_SHAPES), ids=LN_IDS)
def test_layer_norm_against_float64_at_every_geometry(shape, monkeypatch):
    """ops.layer_norm at the shapes of LN_SHAPES: the reduce kernel's batched loop, the NV = 4 variant, 2 / 3 / 32 row groups per
    wave with a row group cut by `ok`, a wave leaving its loop between iterations, a ragged last block.  The cap case
    (4 195 317 rows of 16; nothing smaller has 32 row groups per wave) generates its inputs and takes its float64 reference on
    the device (0.09 s in all on an MI355X, float64 reference included); the others take the CPU reference like
    test_layer_norm_against_float64."""
    dev = _dev()
    ops, _ = _ops()
    monkeypatch.setattr(ops, "LAYERNORM_MIN_ROWS", 0)
    R, D = shape
    geo = H.ln_geometry(R, D)
    t0 = time.perf_counter()
    lg, ref = _layer_norm_pair(D, dev, R + D)
    gd = torch.Generator(device=dev).manual_seed(R + D)
    if shape == H.LN_CAP_SHAPE:
        xg = torch.randn(R, D, generator=gd, device=dev) * 3 + 1.5
        gy = torch.randn(R, D, generator=gd, device=dev)
        ref = ref.to(dev)
        xd, gyd = xg.double().requires_grad_(True), gy.double()
    else:
        g = torch.Generator().manual_seed(R + D)
        x = torch.randn(R, D, generator=g) * 3 + 1.5
        gy = torch.randn(R, D, generator=g)
        xd, gyd = x.double().requires_grad_(True), gy.double()
        xg, gy = x.to(dev), gy.to(dev)
    yd = ref(xd)
    gxd, dgd, dbd = torch.autograd.grad(yd, (xd, ref.weight, ref.bias), gyd)
    yd = yd.detach()
    xg.requires_grad_(True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    y = ops.layer_norm(xg, lg)
    gx, dg, db = torch.autograd.grad(y, (xg, lg.weight, lg.bias), gy, retain_graph=True)
    gx2, dg2, _ = torch.autograd.grad(ops.layer_norm(xg, lg), (xg, lg.weight, lg.bias), gy)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    _rows_close("y", y, yd, H.LN_TOL["y"])
    _rows_close("gx", gx, gxd, H.LN_TOL["gx"])
    parity("dgamma", dg, dgd, tol=H.LN_TOL["dgamma"], kind="scale")
    parity("dbeta", db, dbd, tol=H.LN_TOL["dbeta"], kind="scale")
    assert torch.equal(gx, gx2) and torch.equal(dg, dg2)
    if geo["iters"] > 1:
        # row coverage: integer gradients, exact column sums
        gi = torch.randint(-2, 3, (R, D), generator=gd, device=dev).float()
        _, _, dbi = torch.autograd.grad(y, (xg, lg.weight, lg.bias), gi)
        exact = gi.long().sum(0)
        assert int(exact.abs().max()) < 2 ** 24
        parity("dbeta of integer gy == column sums", dbi, exact, tol=0.0, kind="scale")
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    _WALL[f"{R}x{D}"] = dict(total=t3 - t0, inputs_and_float64_reference=t1 - t0, kernels_forward_and_two_backwards=t2 - t1,
                             comparisons_and_integer_backward=t3 - t2)
    print(f"LayerNorm {R}x{D} iters={geo['iters']}: {t3 - t0:.2f} s (reference {t1 - t0:.2f}, kernels {t2 - t1:.2f}, checks {t3 - t2:.2f})")


@pytest.mark.parametrize("shape", H.LN_RESIDUAL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_layer_norm_residual_form_with_two_row_groups_per_wave(shape, monkeypatch):
    """ops.layer_norm(x, ln, residual=r) (ign_layernorm_res_fwd) with two row groups per wave, a cut row group / a wave that
    stops early: bitwise the two-launch route (torch add, then ign_layernorm_fwd) in the output and all gradients, and the
    `sum` tensor (x + r, the backward's input) written on every row."""
    dev = _dev()
    ops, _lib = _ops()
    monkeypatch.setattr(ops, "LAYERNORM_MIN_ROWS", 0)
    R, D = shape
    lg, _ = _layer_norm_pair(D, dev, R + D + 1)
    gd = torch.Generator(device=dev).manual_seed(R + D + 1)
    x, r, gy = (torch.randn(R, D, generator=gd, device=dev) * 2 + 0.5, torch.randn(R, D, generator=gd, device=dev),
                torch.randn(R, D, generator=gd, device=dev))
    res = {}
    for fused in (True, False):
        xg, rg = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
        y = ops.layer_norm(xg, lg, residual=rg) if fused else ops.layer_norm(xg + rg, lg)
        res[fused] = (y.detach(),) + torch.autograd.grad(y, (xg, rg, lg.weight, lg.bias), gy)
    for name, a, b in zip(("y", "gx", "gr", "dgamma", "dbeta"), res[True], res[False]):
        assert torch.equal(a, b), name
    s = torch.full((R, D), float("nan"), device=dev)
    y, mean, rstd = torch.empty(R, D, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev)
    p = ops._ptr
    _lib.check(_lib.lib().ign_layernorm_res_fwd(p(x), p(r), p(s), p(lg.weight), p(lg.bias), p(y), p(mean), p(rstd), R, D, 1e-5,
                                                ops._stream()), "ign_layernorm_res_fwd")
    torch.cuda.synchronize()
    assert torch.equal(s, x + r) and torch.equal(y, res[True][0])


def test_layer_norm_backward_bound_with_two_row_groups_per_wave():
    """ign_layernorm_bwd_amax at (65545, 64): the slot is max |gx| bit for bit, gx / d(gamma) / d(beta) are those of
    ign_layernorm_bwd"""
    dev = _dev()
    ops, _lib = _ops()
    L, p = _lib.lib(), ops._ptr
    R, D = H.LN_AMAX_SHAPE
    lg, _ = _layer_norm_pair(D, dev, R + D + 2)
    gd = torch.Generator(device=dev).manual_seed(R + D + 2)
    x, gy = torch.randn(R, D, generator=gd, device=dev) * 3 + 1.5, torch.randn(R, D, generator=gd, device=dev)
    y, mean, rstd = torch.empty(R, D, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev)
    _lib.check(L.ign_layernorm_fwd(p(x), p(lg.weight), p(lg.bias), p(y), p(mean), p(rstd), R, D, 1e-5, ops._stream()), "ign_layernorm_fwd")
    nblk = int(L.ign_layernorm_parts(R, D))
    assert nblk == H.ln_geometry(R, D)["nblk"]
    out = []
    for bound in (False, True):
        gx, dg, db = torch.full((R, D), float("nan"), device=dev), torch.empty(D, device=dev), torch.empty(D, device=dev)
        part, slot = torch.empty(nblk * 2 * D, device=dev), torch.zeros(1, device=dev)
        if bound:
            _lib.check(L.ign_layernorm_bwd_amax(p(x), p(gy), p(lg.weight), p(mean), p(rstd), p(gx), p(dg), p(db), p(part), p(slot), R, D,
                                                ops._stream()), "ign_layernorm_bwd_amax")
        else:
            _lib.check(L.ign_layernorm_bwd(p(x), p(gy), p(lg.weight), p(mean), p(rstd), p(gx), p(dg), p(db), p(part), R, D, ops._stream()),
                       "ign_layernorm_bwd")
        out.append((gx, dg, db, slot))
    torch.cuda.synchronize()
    for a, b in zip(out[0][:3], out[1][:3]):
        assert torch.equal(a, b)
    parity("amax slot == max |gx|", out[1][3], out[1][0].abs().max().reshape(1), tol=0.0, kind="scale")
    assert float(out[0][3]) == 0.0


@pytest.mark.parametrize("shape", list(H.LN_FWD_ONLY_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_layer_norm_forward_wider_than_the_backward_takes(shape):
    """ign_layernorm_fwd at D = 2052 (nv = 9) and 4096 (nv = 16): the NV = 16 variant, which ops.layer_norm never reaches (its
    D > 2048 guard; the backward refuses these widths, tests/test_launch_geometry_host.py).  y at the bound of the narrower rows.
    mean, rstd: a lane adds 16 float4 pieces pairwise-then-serially and the row folds over 6 butterfly levels, 24 additions deep;
    the worst-case bound depth * 2^-24 * mean|x| / max|mean| is 2.8e-6 for x = randn * 3 + 1.5 (mean|x| 2.7, max|mean| ~1.6),
    hence 3e-6; the centred squares are positive, so rstd = q^-1/2 carries half of 26 * 2^-24 plus rsqrtf's 2 ulp: 2e-6."""
    dev = _dev()
    ops, _lib = _ops()
    R, D = shape
    lg, ref = _layer_norm_pair(D, dev, R + D)
    g = torch.Generator().manual_seed(R + D)
    x = torch.randn(R, D, generator=g) * 3 + 1.5
    xg = x.to(dev)
    y, mean, rstd = (torch.full((R, D), float("nan"), device=dev), torch.full((R,), float("nan"), device=dev),
                     torch.full((R,), float("nan"), device=dev))
    p = ops._ptr
    _lib.check(_lib.lib().ign_layernorm_fwd(p(xg), p(lg.weight), p(lg.bias), p(y), p(mean), p(rstd), R, D, 1e-5, ops._stream()),
               "ign_layernorm_fwd")
    torch.cuda.synchronize()
    xd = x.double()
    parity("y", y, ref(xd).detach(), tol=H.LN_TOL["y"], kind="scale")
    parity("mean", mean, xd.mean(-1), tol=3e-6, kind="scale")
    parity("rstd", rstd, torch.rsqrt(xd.var(-1, unbiased=False) + 1e-5), tol=2e-6, kind="scale")


# ---------------------------------------------------------------------------------------------------------------- instance norm
@functools.lru_cache(maxsize=None)
def _instnorm_case(shape):
    """-> x (B,T,C) fp32, gy (B,C,T) fp32, and the float64 oracle's xn and input gradient; CPU tensors, computed once, read-only"""
    from oracle import ign_oracle as O
    B, T, C = shape
    x = torch.from_numpy(H.instnorm_input(B, T, C))
    gy = torch.randn(B, C, T, generator=torch.Generator().manual_seed(T + C))
    xd = x.double().requires_grad_(True)
    xn = O.instance_norm(xd)
    gx, = torch.autograd.grad(xn, xd, gy.double())
    return dict(x=x, gy=gy, xn=xn.detach(), gx=gx)


@pytest.mark.parametrize("shape", list(H.INSTNORM_SHAPES), ids=IN_IDS)
def test_instance_norm_forward_at_every_tile_width(shape):
    """xn against float64 at 1e-5 element-wise; the raw transpose bitwise; the input bound exactly max |x|"""
    dev = _dev()
    ops, _ = _ops()
    c = _instnorm_case(shape)
    x = c["x"].to(dev)
    xn, xt = ops.instance_norm(x, want_raw=True, input_bound=True)
    parity("xn", xn, c["xn"], tol=H.XN_TOL, kind="elem")
    assert torch.equal(xt, x.permute(0, 2, 1))
    b = ops.cached_bound(x)
    assert b is not None
    parity("input bound == max |x|", b, x.abs().max().reshape(1), tol=0.0, kind="scale")
    xn0, none = ops.instance_norm(x.clone())
    assert none is None and torch.equal(xn0, xn)


@pytest.mark.parametrize("shape", list(H.INSTNORM_SHAPES), ids=IN_IDS)
def test_instance_norm_backward_at_every_tile_width(shape):
    """autograd through ops.instance_norm (ign_instnorm_bwd) against float64 autograd at 1e-5 of the gradient's maximum (float32
    autograd of the same formula is within 1.3e-7 of float64 at these shapes; the bound leaves the kernel's summation order
    the room the forward needs).  With one constant channel planted in the last -- ragged -- tile, that channel's gradient is
    exactly zero and every other channel's is bitwise what it was."""
    dev = _dev()
    ops, _ = _ops()
    c = _instnorm_case(shape)
    B, T, C = shape
    gy = c["gy"].to(dev)
    x = c["x"].to(dev).requires_grad_(True)
    gx, = torch.autograd.grad(ops.instance_norm(x)[0], x, gy)
    parity("gx", gx, c["gx"], tol=H.GX_TOL, kind="scale")
    xc = c["x"].clone()
    xc[:, :, C - 1] = 50.0
    xc = xc.to(dev).requires_grad_(True)
    xnc = ops.instance_norm(xc)[0]
    gxc, = torch.autograd.grad(xnc, xc, gy)
    assert not gxc[:, :, C - 1].any() and not xnc[:, C - 1].any()
    assert torch.equal(gxc[:, :, :C - 1], gx[:, :, :C - 1])


@pytest.mark.parametrize("shape", list(H.INSTNORM_SHAPES), ids=IN_IDS)
def test_instance_norm_len_at_every_tile_width(shape):
    """ops.instance_norm_len (ign_instnorm_fwd_len) with B = 4 and lengths (T, T // 3 + 1, 1, 0), the padding filled with 1e6:
    each sample is the float64 norm of its truncated self at 1e-5 element-wise, exact zeros from n_b on and for n_b < 2"""
    from oracle import ign_oracle as O
    dev = _dev()
    ops, _ = _ops()
    _, T, C = shape
    lens = [T, T // 3 + 1, 1, 0]
    x = torch.from_numpy(H.instnorm_input(4, T, C, seed=T + 7 * C))
    ref = torch.zeros(4, C, T, dtype=torch.float64)
    for b, n in enumerate(lens):
        x[b, n:] = 1e6
        if n >= 2:
            ref[b, :, :n] = O.instance_norm(x[b:b + 1, :n].double())[0]
    xn = ops.instance_norm_len(x.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev))
    parity("xn", xn, ref, tol=H.XN_TOL, kind="elem")
    for b, n in enumerate(lens):
        assert not xn[b, :, n:].any(), f"sample {b}: padding not exactly zero"
    assert not xn[2].any() and not xn[3].any()
    assert np.isfinite(xn.cpu().numpy()).all()
