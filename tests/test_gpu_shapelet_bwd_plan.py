"""The shapelet weight backward against float64 at every branch of its launch plan.  The rows, the Python restatement of
plan_bwd / plan_bwd_strided and the proof that each row reaches its branch are in tests/shapelet_bwd_plan_cases.py and
tests/test_shapelet_bwd_plan_host.py (no GPU); this file runs them.

Every row runs ops.shapelet_bank forward and backward with a seeded upstream gradient on BOTH host routes -- the bank entry
points (ign_shapelet_bwd_bank: reduce_bank_kernel, which ops takes for up to 8 groups) and the per-group entry points
(ign_shapelet_bwd: ign_launch_reduce_parts with its three kernels; ops.BANK_MAX_GROUPS = 0 sends a bank there) -- and compares
p and d_min (1e-4 element-wise) and grad_w, with LTS also the threshold gradient (1e-4 of the tensor's own scale: _close /
_grad_close of tests/test_gpu_shapelet.py, nothing looser) with the float64 oracle; the backward runs twice and must repeat bit
for bit; up to 128 batch slices the two routes must agree bit for bit, above (B = 257, 259) reduce_bank_kernel keeps four slices
where the per-group reducer takes sixteen, so there both are held against float64 only.  The inputs are tie-free
(shapelet_bwd_plan_cases.inputs), which keeps the sign(0) convention of the L1 kernels out of the comparison.

The capped row (64 x 122 x 2048, K = 10, L = 2000: 156 MB of partials) takes its reference on two channels, the first and the
last: a weight gradient at channel c depends on x[:, c] and g[:, :, c] only; those slices alone are compared, every other
channel is checked to be finite and written.  Rows whose 5-D broadcast exceeds a few million elements take the float64 oracle on
the device (the same torch code).

Observed on an MI355X (profiles/shapelet_bwd_plan.json), as fractions of the tolerance: grad_w 0.017 at most (seven window
chunks), p 0.015 and d_min 0.016 (strided, two j-tiles), threshold gradient 0.0012; the routes differ above 128 slices and nowhere
else; the slowest row (capped) takes 0.73 s with its reference.

IGN_SHAPELET_BWD_PLAN_OUT=<file>: observed errors (as multiples of the tolerance) and wall times of every row are written there
as JSON; tests/diag_shapelet_bwd_plan.py merges them into profiles/shapelet_bwd_plan.json."""
import functools
import json
import os
import time

import pytest
import torch

import shapelet_bwd_plan_cases as T
import test_shapelet_bwd_plan_host as H
from conftest import parity

pytestmark = pytest.mark.gpu
_REC = {}
LIVE = [c for c in T.CASES if c[0] != "refused"]


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("IGN_SHAPELET_BWD_PLAN_OUT")
    if _REC and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(gpu_rows=_REC), f, indent=1, sort_keys=True)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ops():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ops
    return ops, _lib


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    """-> dict(xn, w, thr, r: fp32 CPU inputs; P, D, gw, gt: the float64 oracle's, restricted to `channels` where that is set;
    cols: the columns of P / D the reference holds).  Computed once per process, read-only."""
    _, (B, C, T_, K, L, stride), mode, _, _ = T.BY_ID[case_id]
    xn, w, thr, r = T.inputs(case_id)
    T.assert_no_ties(xn, w)
    ch = torch.tensor(T.CAPPED_CHANNELS) if case_id == "capped" else torch.arange(C)
    cols = (torch.arange(K)[:, None] * C + ch[None, :]).reshape(-1)                      # feature order k*C + c
    Tw = (T_ - L) // stride + 1
    big = B * Tw * K * len(ch) * L > 4_000_000
    t0 = time.perf_counter()
    P, D, gw, gt = T.oracle(xn[:, ch], w[:, ch], thr[:, :, ch], r[:, cols], mode, stride,
                            device=torch.device("cuda:0") if big else None)
    return dict(xn=xn, w=w, thr=thr, r=r, P=P, D=D, gw=gw, gt=gt, ch=ch, cols=cols, seconds=time.perf_counter() - t0,
                oracle_on="device" if big else "cpu")


def _run(ops, dev, ref, mode, stride):
    """forward + backward through ops.shapelet_bank on the route ops is set to -> (P, D, grad_w, grad_thr or None)"""
    w = ref["w"].to(dev).requires_grad_(True)
    thr = ref["thr"].to(dev).requires_grad_(True)
    lts = bool(mode & T.LTS)
    P, D = ops.shapelet_bank(ref["xn"].to(dev), [w], T.EPS, mode, [stride], [thr] if lts else None)
    grads = torch.autograd.grad((P * ref["r"].to(dev)).sum(), [w] + ([thr] if lts else []))
    return P.detach(), D, grads[0], (grads[1] if lts else None)


def _compare(tag, ref, out, lts):
    """the four comparisons of a row against float64, on the reference's channels -> {tensor: error over tolerance}"""
    P, D, gw, gt = out
    ch, cols = ref["ch"], ref["cols"]
    recs = dict(p=parity(f"{tag} p", P.cpu()[:, cols], ref["P"], tol=T.VAL_TOL, kind="elem", ref_is="oracle float64"),
                dmin=parity(f"{tag} dmin", D.cpu()[:, cols], ref["D"], tol=T.VAL_TOL, kind="elem", ref_is="oracle float64"),
                grad_w=parity(f"{tag} grad_w", gw.cpu()[:, ch], ref["gw"], tol=T.GRAD_TOL, kind="scale", floor=T.GRAD_FLOOR,
                              ref_is="oracle float64"))
    if lts:
        recs["grad_thr"] = parity(f"{tag} grad_thr", gt.cpu()[:, :, ch], ref["gt"], tol=T.GRAD_TOL, kind="scale", floor=T.GRAD_FLOOR,
                                  ref_is="oracle float64")
    return {k: v["err_over_1e4"] for k, v in recs.items()}


@pytest.mark.parametrize("case", LIVE, ids=[c[0] for c in LIVE])
def test_row_against_float64_on_both_routes(case, monkeypatch):
    dev = _dev()
    ops, _lib = _ops()
    case_id, shape, mode, branch, _ = case
    B, C, T_, K, L, stride = shape
    plan = H.plan_bwd(*shape)
    got = H.lib_plan(_lib.lib(), shape)
    assert got == {k: plan[k] for k in H.PLAN_FIELDS}                        # the library plans what the table was built on
    t0 = time.perf_counter()
    ref = _reference(case_id)
    lts = bool(mode & T.LTS)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    bank = _run(ops, dev, ref, mode, stride)
    again = _run(ops, dev, ref, mode, stride)
    monkeypatch.setattr(ops, "BANK_MAX_GROUPS", 0)                           # a bank of one then goes group by group
    group = _run(ops, dev, ref, mode, stride)
    monkeypatch.undo()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    errs = dict(bank=_compare("bank", ref, bank, lts), per_group=_compare("per-group", ref, group, lts))
    for a, b in zip(bank, again):
        assert a is None or torch.equal(a, b), "the backward is not bitwise repeatable"
    assert torch.equal(bank[0], group[0]) and torch.equal(bank[1], group[1])
    same = torch.equal(bank[2], group[2])
    if plan["nbs"] <= 128:
        assert same, "bank and per-group gradients differ below 129 batch slices"
    if ref["ch"].numel() < C:
        # the channels without a reference: finite, and every row written (each entry sums thousands of non-zero terms)
        assert torch.isfinite(bank[2]).all() and float(bank[2].abs().amax(dim=2).min()) > 0.0
    _REC[case_id] = dict(shape=list(shape), mode=mode, branch=branch, errors_over_tol=errs, routes_bitwise_equal=same,
                         oracle_on=ref["oracle_on"], reference_channels=ref["ch"].tolist(),
                         seconds=dict(total=time.perf_counter() - t0, inputs_and_float64_reference=t1 - t0,
                                      three_forward_backward_runs=t2 - t1))
    print(f"{case_id} {shape} mode 0x{mode:02x} nbs={plan['nbs']}: bank {errs['bank']} per-group {errs['per_group']} "
          f"bitwise equal routes: {same}  [{time.perf_counter() - t0:.2f} s]")


@pytest.mark.parametrize("B", [33, 75])
def test_two_group_bank_equals_the_per_group_calls_bit_for_bit(B, monkeypatch):
    """nbs = 17 and 38 with two length groups (JJ = 4 and JJ = 8) in ONE ign_shapelet_bwd_bank call: the nparts >= 16 branch of
    reduce_bank_kernel with blockIdx.y > 0 and groups of different size, against two ign_shapelet_bwd calls
    (reduce_parts_x4_kernel) bit for bit, and against the float64 oracle group by group"""
    dev = _dev()
    ops, _ = _ops()
    C, T_, Ks, Ls = 2, 100, (3, 5), (8, 60)
    assert [H.plan_bwd(B, C, T_, K, L)["nbs"] for K, L in zip(Ks, Ls)] == [(B + 1) // 2] * 2
    gen = torch.Generator().manual_seed(B)
    xn = (torch.randn(B, C, T_, generator=gen).view(torch.int32) & ~1).view(torch.float32)
    ws = [(torch.randn(K, C, L, generator=gen).view(torch.int32) | 1).view(torch.float32) for K, L in zip(Ks, Ls)]
    r = torch.randn(B, sum(Ks) * C, generator=gen)
    for w in ws:
        T.assert_no_ties(xn, w)

    def run():
        wd = [w.to(dev).requires_grad_(True) for w in ws]
        P, _ = ops.shapelet_bank(xn.to(dev), wd, T.EPS, T.L1 | T.RBF)
        return [P.detach()] + list(torch.autograd.grad((P * r.to(dev)).sum(), wd))

    one_call = run()
    monkeypatch.setattr(ops, "BANK_MAX_GROUPS", 0)
    per_group = run()
    monkeypatch.undo()
    for a, b in zip(one_call, per_group):
        assert torch.equal(a, b)
    col = 0
    for g, w in enumerate(ws):
        n = Ks[g] * C
        _, _, gw, _ = T.oracle(xn, w, torch.zeros(1, Ks[g], C), r[:, col:col + n], T.L1 | T.RBF, 1)
        parity(f"B{B} group {g} grad_w", one_call[1 + g], gw, tol=T.GRAD_TOL, kind="scale", floor=T.GRAD_FLOOR, ref_is="oracle float64")
        col += n


def test_refused_shape_raises_without_a_launch():
    """L = 4100 at stride 1: the forward runs, the backward has no plan -- both routes raise, and the timing registry shows that
    neither the backward kernel nor a reducer was launched"""
    dev = _dev()
    ops, _lib = _ops()
    _, (B, C, T_, K, L, stride), mode, _, _ = T.BY_ID["refused"]
    assert H.lib_plan(_lib.lib(), (B, C, T_, K, L, stride)) == H.E_TOOBIG
    gen = torch.Generator().manual_seed(1)
    xn = torch.randn(B, C, T_, generator=gen).to(dev)
    _lib.timing_enable(True)
    try:
        for groups in (ops.BANK_MAX_GROUPS, 0):
            w = torch.randn(K, C, L, generator=gen).to(dev).requires_grad_(True)
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(ops, "BANK_MAX_GROUPS", groups)
                P, _ = ops.shapelet_bank(xn, [w], T.EPS, mode)
                with pytest.raises(_lib.IgnError, match="no launch plan"):
                    P.sum().backward()
            assert w.grad is None
        torch.cuda.synchronize()
        assert _lib.timing_read("shp_fwd")[1] > 0
        assert _lib.timing_read("shp_bwd")[1] == 0 and _lib.timing_read("reduce_parts")[1] == 0
    finally:
        _lib.timing_enable(False)
