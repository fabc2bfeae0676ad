"""What tests/bn_elu_pool_cases.py claims, checked without a GPU: its constants are those of csrc/ign_eegcnn_fused.hip; its table
reaches every class of every plan, every regime is what its name says, the eps-dominated rows really have a first-order dalpha and the
exact rows really are exact; an fp32 restatement of the kernels meets every tolerance with 4x headroom in every regime; every seeded
defect fails a row that names the class it breaks while the control defect passes; and the numpy references are float64 torch
autograd through BatchNorm2d -> elu -> avg_pool2d."""
import os
import re

import numpy as np
import pytest

import bn_elu_pool_cases as K

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-imagery-eeg_amd", "csrc", "ign_eegcnn_fused.hip")
HEADROOM = 0.25


def _ids(cs):
    return [c.id for c in cs]


def _kernel(src, name):
    m = re.search(r"__global__ void (__launch_bounds__\((\d+)\) )?" + name + r"\(.*?\n}\n", src, re.S)
    assert m, name
    return m.group(0), (int(m.group(2)) if m.group(2) else None)


def test_constants_are_those_of_the_source():
    src = open(SRC).read()
    for name in ("chan_stats_kernel", "affine_elu_pool_kernel", "bn_elu_pool_bwd_sums_kernel", "bn_elu_pool_bwd_apply_kernel"):
        body, bound = _kernel(src, name)
        assert bound == K.THREADS, name
        assert re.search(rf"(\+= {K.THREADS}\b|\* {K.THREADS} \+ threadIdx\.x)", body), name
    assert re.search(rf"static int stat_slices\(int B\) \{{ return std::max\(1, std::min\(B, {K.SLICE_CAP}\)\); \}}", src)
    for name in ("bn_fold_fwd_kernel", "bn_fold_bwd_kernel"):
        assert len(re.findall(rf"hipLaunchKernelGGL\({name}, dim3\(\(unsigned\)\(\(C \+ {K.FOLD_BLOCK - 1}\) / {K.FOLD_BLOCK}\)\), "
                              rf"dim3\({K.FOLD_BLOCK}\)", src)) == 1, name
    fin = re.findall(r"hipLaunchKernelGGL\(chan_stats_finalize_kernel, dim3\(\(unsigned\)\(\(2 \* Cc \+ (\d+)\) / (\d+)\)\), dim3\((\d+)\)", src)
    assert fin == [(str(K.FIN_BLOCK - 1), str(K.FIN_BLOCK), str(K.FIN_BLOCK))] * 2
    launches = re.findall(r"hipLaunchKernelGGL\((chan_stats_kernel|affine_elu_pool_kernel|bn_elu_pool_bwd_sums_kernel|"
                          r"bn_elu_pool_bwd_apply_kernel), dim3\((.*?)\), dim3\((\d+)\)", src)
    assert len(launches) == 4 and all(int(t) == K.THREADS for _, _, t in launches)
    chk = re.search(r"static int bn_check\(.*?\n}\n", src, re.S).group(0)
    assert ("B <= 0 || Cc <= 0 || T <= 0 || P <= 0 || P > T || "
            f"Cc > {K.BN_C_MAX} || (long long)B * Cc > {K.BN_BC_MAX}LL || T > 65535 * 256") in chk
    assert K.BN_T_MAX == 65535 * 256 and "return IGN_E_ARG;" in chk
    hdr = open(os.path.join(os.path.dirname(SRC), "..", "..", "include", "ign_hip.h")).read() if os.path.exists(
        os.path.join(os.path.dirname(SRC), "..", "..", "include", "ign_hip.h")) else None
    if hdr and "IGN_E_ARG" in hdr:
        assert re.search(rf"IGN_E_ARG\s*=?\s*\(?{K.IGN_E_ARG}\b", hdr)
    for B, C, T, P, want in ((2, 3, 10, 10, False), (2, 3, 10, 11, True), (2, 3, 10, 0, True), (1, 65536, 1, 1, True), (1, 65535, 1, 1, False)):
        assert K.bn_refuses(B, C, T, P) == want
    assert all(K.bn_refuses(r["B"], r["C"], r["T"], r["P"]) for r in K.REFUSALS)


def test_table_reaches_every_class_and_every_axis_value():
    cs = K.cases()
    assert 40 <= len(cs) <= 150
    hit = set().union(*[K.plan(c)["classes"] for c in cs])
    assert K.all_classes() - hit == set(), sorted(K.all_classes() - hit)
    assert max(c.B * c.C * c.T for c in cs) <= 2e6
    assert {c.B for c in cs} >= {1, 2, 31, 32, 33, 64, 65}
    assert {c.C for c in cs} >= {1, 3, 63, 64, 65, 129}
    assert {c.T for c in cs} >= {2, 63, 64, 65, 255, 256, 257, 513, 1285}
    assert {c.P for c in cs} >= {1, 2, 5} and any(c.P == c.T for c in cs)
    assert {c.regime for c in cs} == set(K.OP_REGIMES) | set(K.DIRECT_REGIMES)
    assert any(K.plan_pool(c.T, c.P)["Tp"] == 257 and c.P == 5 for c in cs)
    assert {1, 2} <= set().union(*[K.plan_stats(c.B, c.C, c.T)["rows_per_slice"] for c in cs if c.B == 33])
    assert {2, 3} == set().union(*[K.plan_stats(c.B, c.C, c.T)["rows_per_slice"] for c in cs if c.B == 65])
    assert any(not c.affine for c in cs) and all(c.affine for c in cs if c.regime != "gauss")
    for d_, cls in K.DEFECTS.items():
        assert any(cls in K.plan(c)["classes"] for c in cs), d_


@pytest.mark.parametrize("c", [c for c in K.cases() if c.regime.startswith("epsdom")], ids=lambda c: c.id)
def test_eps_dominated_rows_have_a_first_order_dalpha(c):
    R = K.reference_op(c)
    da, dg = np.abs(R["dalpha"].ref).max(), np.abs(R["dgamma"].ref).max()
    assert da >= K.MIN_DALPHA_OVER_DGAMMA * dg, (da, dg)
    d = K.inputs(c)
    assert (d["alpha"] > 0).any() and (d["alpha"] < 0).any()
    # no floor: the bound is made of dalpha's own terms and stays far below dalpha itself, let alone dgamma
    assert R["dalpha"].tol.max() <= 1e-3 * da


@pytest.mark.parametrize("c", [c for c in K.cases() if c.regime in ("constant", "zero_crossing", "saturated", "exact")
                               or c.regime.startswith("offset")], ids=lambda c: c.id)
def test_regimes_are_what_they_say(c):
    d = K.inputs(c)
    v = d["v"]
    if c.regime == "constant":
        sums = K.restate_stats(v)
        n = c.B * c.T
        m = sums[:, 0] / n
        raw = sums[:, 1] / n - m * m
        assert raw[0] == 0.0 and raw[1] == -K.CONST_SHORTFALL          # the clamp is taken, by exactly -2^-26
        assert d["eps"] < K.CONST_SHORTFALL * float(d["alpha"][1]) ** 2
        R = K.reference_op(c)
        assert R["dgamma"].ref[0] == 0 and R["dgamma"].ref[1] == 0 and R["dalpha"].ref[1] == 0
    elif c.regime.startswith("offset"):
        x = v.astype(np.float64)
        ratio = np.abs(x.mean(axis=(0, 2))) / x.std(axis=(0, 2))
        assert (np.abs(ratio / float(c.regime[6:]) - 1) < 0.25).all()
    else:
        z = K.fma32(d["scale"][None, :, None], v, d["shift"][None, :, None])
        if c.regime == "zero_crossing":
            assert 0.2 <= float((z == 0).mean()) <= 0.3 and (z > 0).any() and (z < 0).any()
            assert (K.elu_grad32(z)[z == 0] == 1).all()
        elif c.regime == "saturated":
            assert z.max() <= -20 and z.min() < -88                     # expm1f saturates; __expf underflows in some elements
        else:
            assert z.min() > 0 and c.P & (c.P - 1) == 0
            assert all((d[k] == np.round(d[k])).all() for k in ("v", "dout", "mean", "kb"))


@pytest.mark.parametrize("c", K.cases(), ids=lambda c: c.id)
def test_restatement_meets_every_tolerance_with_headroom(c):
    """... and equals float64 where the tolerance is 0 (the exact rows)"""
    give, refs = K.direct(c)
    got = K.restate_direct(c, give)
    bad = []
    for entry, outs in refs.items():
        for k, r in outs.items():
            q = K.ratio(got[entry][k], r)
            if c.exact and entry in ("ign_chan_stats", "ign_affine_elu_pool_fwd", "ign_bn_elu_pool_bwd_sums", "ign_bn_elu_pool_bwd_apply"):
                assert not (r.tol > 0).any(), (entry, k)
            if not q <= HEADROOM:
                bad.append((entry, k, q))
    if not c.direct:
        R, g = K.reference_op(c), K.restate_op(c)
        for k, r in R.items():
            q = K.ratio(g[k], r)
            if not q <= HEADROOM:
                bad.append(("op", k, q))
        assert ("dalpha" in R) == c.affine
    assert not bad, bad


def _fails(c, defect, **kw):
    R, g = K.reference_op(c, **kw), K.restate_op(c, defect, **kw)
    return sorted(k for k in K.OP_OUTPUTS if k in R and not K.ratio(g[k], R[k]) <= 1.0)


@pytest.mark.parametrize("defect", sorted(K.DEFECTS))
def test_every_seeded_defect_fails_a_row_of_its_class(defect):
    cls = K.DEFECTS[defect]
    rows = [c for c in K.op_cases() if cls in K.plan(c)["classes"] and c.regime in ("gauss", "epsdom_small", "epsdom_eps")
            and (c.affine or "dalpha" not in defect)]
    assert rows
    failed = {c.id: _fails(c, defect) for c in rows[:6]}
    assert any(failed.values()), failed
    if "dalpha" in defect:          # seen in EVERY row with an alpha, the Gaussian ones included, and through dalpha itself
        assert all("dalpha" in f for f in failed.values()), failed
    # and no row outside the class is touched by a defect that is about launch geometry
    if defect in ("strided_rows", "remainder_dv_zero"):
        clean = [c for c in K.op_cases() if cls not in K.plan(c)["classes"] and c.regime == "gauss"][:3]
        assert all(_fails(c, defect) == [] for c in clean)


def test_control_defect_is_not_flagged_in_the_gauss_rows():
    """kb from the mean rounded to fp32 is within the bound at |mean| / sigma ~ 0.2 ..."""
    rows = [c for c in K.op_cases() if c.regime == "gauss"][:8]
    assert all(_fails(c, K.CONTROL_DEFECT) == [] for c in rows)


def test_case_module_is_numpy_only():
    src = open(K.__file__).read()
    assert not re.search(r"^\s*(import|from) torch", src, re.M)


TORCH_ROWS = [c for c in K.op_cases() if (c.B, c.C, c.T, c.P) in ((2, 3, 63, 2), (31, 3, 65, 5), (2, 1, 64, 1), (33, 5, 257, 1))]


@pytest.mark.parametrize("c", TORCH_ROWS, ids=lambda c: c.id)
@pytest.mark.parametrize("momentum", [None, "cumulative"])
def test_numpy_references_are_float64_torch_autograd(c, momentum):
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    d = K.inputs(c)
    R = K.reference_op(c, momentum=momentum, calls=2)
    bn = torch.nn.BatchNorm2d(c.C, eps=d["eps"], momentum=None if momentum else d["momentum"]).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(d["gamma"]))
        bn.bias.copy_(torch.from_numpy(d["beta"]))
        bn.running_mean.copy_(torch.from_numpy(d["run_mean"]))
        bn.running_var.copy_(torch.from_numpy(d["run_var"]))
    v = torch.from_numpy(d["v"]).double().requires_grad_(True)
    a = torch.from_numpy(d["alpha"]).double().requires_grad_(True) if c.affine else None
    cs = torch.from_numpy(d["cshift"]).double().requires_grad_(True) if c.affine else None
    for _ in range(2):
        y = v * a.view(1, -1, 1) + cs.view(1, -1, 1) if c.affine else v
        out = F.avg_pool2d(F.elu(bn(y.unsqueeze(2))), (1, c.P)).squeeze(2)
    grads = torch.autograd.grad((out * torch.from_numpy(d["dout"]).double()).sum(), [v, bn.weight, bn.bias] + ([a, cs] if c.affine else []))
    got = dict(out=out, dv=grads[0], dgamma=grads[1], dbeta=grads[2], run_mean=bn.running_mean, run_var=bn.running_var)
    if c.affine:
        got["dalpha"] = grads[3]
        assert float(grads[4].abs().max()) <= 1e-9 * max(1.0, float(grads[1].abs().max()))          # dc = 0 up to float64 rounding
    for k, t in got.items():
        ref, x = R[k].ref, t.detach().numpy()
        scale = np.abs(ref).max()
        if k == "dalpha":       # autograd has no closed form: it sums dy v = dv v / alpha over the batch, terms that cancel down to
            # the eps-sized remainder, so ITS float64 rounding is relative to those terms (the closed form has no cancellation)
            scale = ((np.abs(R["dv"].ref) * np.abs(d["v"].astype(np.float64))).sum(axis=(0, 2)) / np.abs(d["alpha"].astype(np.float64))).max()
        assert np.abs(x - ref).max() <= 1e-12 * max(scale, 1e-300), (k, np.abs(x - ref).max(), scale)


@pytest.mark.parametrize("c", [c for c in TORCH_ROWS if c.regime == "gauss"], ids=lambda c: c.id)
def test_numpy_eval_reference_is_float64_torch_autograd(c):
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    d = K.inputs(c)
    R = K.reference_eval(c)
    bn = torch.nn.BatchNorm2d(c.C, eps=d["eps"]).double().eval()
    with torch.no_grad():
        for p_, k in ((bn.weight, "gamma"), (bn.bias, "beta"), (bn.running_mean, "run_mean"), (bn.running_var, "run_var")):
            p_.copy_(torch.from_numpy(d[k]))
    v = torch.from_numpy(d["v"]).double().requires_grad_(True)
    leaves = [v, bn.weight, bn.bias]
    y = v
    if c.affine:
        a, cs = (torch.from_numpy(d[k]).double().requires_grad_(True) for k in ("alpha", "cshift"))
        y = v * a.view(1, -1, 1) + cs.view(1, -1, 1)
        leaves += [a, cs]
    out = F.avg_pool2d(F.elu(bn(y.unsqueeze(2))), (1, c.P)).squeeze(2)
    grads = torch.autograd.grad((out * torch.from_numpy(d["dout"]).double()).sum(), leaves)
    got = dict(zip(("dv", "dgamma", "dbeta", "dalpha", "dc"), grads), out=out)
    assert set(got) == set(R)
    for k, t in got.items():
        ref = R[k].ref
        assert np.abs(t.detach().numpy() - ref).max() <= 1e-12 * np.abs(ref).max(), k
