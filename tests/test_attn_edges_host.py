"""Attention edge tests, host side: the table of tests/attn_edge_cases.py meets every tail class on every (arithmetic, head width)
route, each route is the one ops._attn_arith picks, the geometry constants are the kernel sources', the regime inputs are what they
claim in float64, the regime tolerances obey their condition, and the wrapper's operand rule copies what the kernels refuse.
The GPU side is tests/test_gpu_attn_edges.py."""
import os
import re

import pytest
import torch

import attn_edge_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech-imagery-eeg_amd", "csrc")


def _ops():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    return ops


# ----------------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("amath,E", C.ROUTES)
def test_every_route_meets_every_tail_class(amath, E):
    """The table is shared by all routes, so the L and S classes are route-independent; the branch classes are computed from the
    tile sizes of the kernels the route runs."""
    Ls, Ss = {L for L, _ in C.EDGE_PAIRS}, {S for _, S in C.EDGE_PAIRS}
    for name, pred in C.L_CLASSES.items():
        assert any(pred(L) for L in Ls), f"no L of class {name!r}"
    for name, pred in C.S_CLASSES.items():
        assert any(pred(S) for S in Ss), f"no S of class {name!r}"
    for name, pred in C.branch_classes(amath, E).items():
        assert any(pred(L, S) for L, S in C.EDGE_PAIRS), f"{amath} E={E}: no pair reaches {name!r}"


def test_the_classes_are_the_ones_the_issue_lists():
    assert sorted(L for L in range(1, 200) if any(p(L) for n, p in C.L_CLASSES.items() if not n.startswith("above"))) \
        == [1, 31, 32, 33, 127, 128, 129]
    assert C.L_CLASSES["above workgroup + wave"](161) and not C.L_CLASSES["above workgroup + wave"](160)
    exact = sorted(S for S in range(1, 200) if any(p(S) for n, p in C.S_CLASSES.items() if not n.startswith("below")))
    assert exact == [1, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129]
    assert [S for S in range(1, 200) if C.S_CLASSES["below one score tile"](S)] == list(range(2, 32))


def test_route_list():
    assert len(C.ROUTES) == len(set(C.ROUTES)) == 14
    for amath in ("f32", "bf16x6"):
        assert {E for a, E in C.ROUTES if a == amath} == {16, 32, 64, 128}
    for amath in ("f16x3", "bf16"):
        assert {E for a, E in C.ROUTES if a == amath} == {16, 32, 64}
    # every regime case is a route; every pair list is part of the table
    assert {(a, E) for _, a, E in C.regime_routes()} == {(a, E) for a, E in C.ROUTES if E in C.REGIME_WIDTHS}
    assert set(C.DROPOUT_PAIRS) <= set(C.EDGE_PAIRS) and set(C.UNROUTED_PAIRS) <= set(C.EDGE_PAIRS)


@pytest.mark.parametrize("amath,E", C.ROUTES + [("f16x3", 128)])
def test_route_is_the_one_attn_arith_returns(amath, E, monkeypatch):
    ops = _ops()
    assert (ops.ATTN_MATH_F32, ops.ATTN_MATH_X6, ops.ATTN_MATH_BF16, ops.ATTN_MATH_H3) == \
        (C.ATTN_MATH_F32, C.ATTN_MATH_X6, C.ATTN_MATH_BF16, C.ATTN_MATH_H3)
    attn_math, gemm_math, autocast = C.knobs(amath)
    monkeypatch.setattr(ops, "ATTN_MATH", attn_math)
    monkeypatch.setattr(ops, "GEMM_MATH", gemm_math)
    route = "bf16x6" if (amath, E) == ("f16x3", 128) else amath
    assert (ops._attn_arith(E, autocast, False, True), ops._attn_arith(E, autocast, True)) == C.route_arith(route, E)
    assert ops._attn_arith(E, autocast, False) == ops._attn_arith(E, autocast, False, False) == C.inference_arith(route, E)
    if E == 128:                                                        # autocast does not reach the single-product kernels there
        assert ops._attn_arith(E, True, False) != C.ATTN_MATH_BF16


def test_a_differentiated_call_keeps_forward_and_backward_in_one_kernel_family(monkeypatch):
    """The backward forms its probabilities from its own scores and the forward's lse: every route pairs a forward and a backward
    of the same family (at E = 128 under the split arithmetics the fp32-MFMA pair), a call that is not differentiated keeps the
    faster split forward."""
    ops = _ops()
    for amath, E in C.ROUTES + [("f16x3", 128)]:
        attn_math, gemm_math, autocast = C.knobs(amath)
        monkeypatch.setattr(ops, "ATTN_MATH", attn_math)
        monkeypatch.setattr(ops, "GEMM_MATH", gemm_math)
        assert ops._attn_arith(E, autocast, False, True) == ops._attn_arith(E, autocast, True), (amath, E)
        if amath != "f32" and E == 128:
            assert ops._attn_arith(E, autocast, False) == C.ATTN_MATH_X6


# ----------------------------------------------------------------------------------------------------------------- the sources
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _constexpr(src, name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src)
    assert m, f"constexpr int {name} not found"
    return int(m.group(1))


def test_constants_equal_the_kernel_sources():
    f32, x6, mp = _src("ign_attention.hip"), _src("ign_attention_x6.hip"), _src("ign_attention_map.hip")
    assert _constexpr(f32, "ATT_KT") == C.ATT_KT
    assert _constexpr(mp, "MAP_KT") == C.MAP_KT
    assert _constexpr(x6, "AB_T") == C.AB_T
    m = re.search(r"static\s+constexpr\s+int\s+KT\s*=\s*E\s*==\s*(\d+)\s*\?\s*(\d+)\s*:\s*(\d+)\s*;", x6)
    assert m, "AxPitch<E>::KT not found"
    e0, kt0, kt1 = map(int, m.groups())
    for E in C.HEAD_WIDTHS:
        assert C.x6_key_tile(E) == (kt0 if E == e0 else kt1)
    # queries (keys in dK / dV) per workgroup and per wave: every kernel indexes blockIdx.x * 128 + wave * 32
    for name, src, n in (("ign_attention.hip", f32, 3), ("ign_attention_x6.hip", x6, 3), ("ign_attention_map.hip", mp, 1)):
        found = re.findall(r"blockIdx\.x\s*\*\s*(\d+)\s*\+\s*wave\s*\*\s*(\d+)", src)
        assert len(found) == n, (name, found)
        assert set(found) == {(str(C.WG_QUERIES), str(C.WAVE_QUERIES))}, (name, found)
    assert C.DKV_WG_KEYS == C.WG_QUERIES
    for src in (f32, x6):
        assert re.search(r"\(\s*S\s*\+\s*127\s*\)\s*/\s*128", src) and re.search(r"\(\s*L\s*\+\s*127\s*\)\s*/\s*128", src)
    # 32-key score tiles: the sub-tile loops step by 32 and the x6 forward masks by kt0 + kb + 32 > S
    assert "ATT_KT / 32" in f32 and "AX_KT / 32" in x6 and "MAP_KT / 32" in mp and C.SUB_KEYS == 32
    assert re.search(r"kt0\s*\+\s*kb\s*\+\s*32\s*>\s*a\.S", x6)
    widths = re.search(r"E\s*!=\s*16\s*&&\s*E\s*!=\s*32\s*&&\s*E\s*!=\s*64\s*&&\s*E\s*!=\s*128", x6)
    assert widths and C.HEAD_WIDTHS == (16, 32, 64, 128)


def test_bounds_equal_the_tests_they_come_from():
    base = open(os.path.join(ROOT, "tests", "test_gpu_baselines.py")).read()
    assert 'assert _rel(o, oref) < 2e-5, "forward"' in base and "assert _rel(a, b) < 5e-5, name" in base
    assert (C.FWD_TOL, C.GRAD_TOL) == (2e-5, 5e-5)
    mp = open(os.path.join(ROOT, "tests", "test_gpu_attn_map.py")).read()
    assert '< 1e-5, "rows of the p = 0 map sum to 1"' in mp
    assert '(1e-4 if amath == "bf16" else 2e-5), "map vs float64"' in mp
    assert '(3e-2 if amath == "bf16" else 2e-5), "attn @ v vs out"' in mp
    assert C.MAP_ROWSUM_TOL == 1e-5 and C.MAP_TOL == {"bf16": 1e-4} and C.MAP_OUT_TOL == {"bf16": 3e-2}
    dr = open(os.path.join(ROOT, "tests", "test_gpu_attn_dropout.py")).read()
    assert "1e-4 < _rel(o, oref) < 3e-2" in dr and "assert _rel(a, b) < 5e-2, name" in dr
    assert (C.BF16_DROPOUT_FWD_TOL, C.BF16_DROPOUT_GRAD_TOL) == (3e-2, 5e-2)


# ----------------------------------------------------------------------------------------------------------------- the metric
def test_slice_metric_sees_a_defect_in_a_small_slice():
    ref = torch.ones(2, 5, 3, 4, dtype=torch.float64)
    ref[0, :, 0] *= 1000.0
    got = ref.clone()
    got[1, 2, 1, 3] += 1e-3
    assert C.whole_err(got, ref) == pytest.approx(1e-6)
    assert C.slice_err(got, ref) == pytest.approx(1e-3)
    # identically zero reference: exact zeros pass, anything else is judged against the floor
    z = torch.zeros(1, 2, 1, 4)
    assert C.slice_err(z, z) == 0.0
    assert C.slice_err(z + 1e-9, z) == float("inf")
    assert C.slice_err(z + 1e-3, z, floor=10.0) == pytest.approx(1e-4)
    assert C.slice_err(z * float("nan"), z) == float("inf")
    m = torch.rand(2, 3, 5, 7, dtype=torch.float64)
    assert C.slice_err(m * (1 + 1e-6), m, dims=(2, 3)) == pytest.approx(1e-6, rel=1e-3)


def test_zero_floors():
    q, k, v, go = C.edge_inputs(129, 1, 16)
    fl = C.zero_floors(q, k, v, go, 0.25, 1)
    nat = 0.25 * 16 * float(go.abs().max()) * float(v.abs().max())
    assert fl == {"dq": nat * float(k.abs().max()), "dk": nat * float(q.abs().max())}
    assert C.zero_floors(q, k, v, go, 0.25, 2) == {}
    ref = C.edge_reference(129, 1, 16)
    assert float(ref["dq"].abs().max()) == 0.0 and float(ref["dk"].abs().max()) == 0.0 and float(ref["dv"].abs().max()) > 0
    for L, S in C.EDGE_PAIRS:
        if S > 1:
            r = C.edge_reference(L, S, 16)
            assert float(r["dq"].abs().amax((1, 3)).min()) > 0 and float(r["dk"].abs().amax((1, 3)).min()) > 0, (L, S)


def test_edge_inputs_have_the_stated_batch_and_heads():
    for E in C.HEAD_WIDTHS:
        B, H = C.batch_heads(E)
        assert (B, H) == ((1, 2) if E == 128 else (2, 3))
        q, k, v, go = C.edge_inputs(33, 31, E)
        assert q.shape == go.shape == (B, 33, H, E) and k.shape == v.shape == (B, 31, H, E)


# ----------------------------------------------------------------------------------------------------------------- the regimes
def _scores(name, E, bf16=False):
    q, k, v, go = C.regime_inputs(name, E, bf16)
    return C.scale_of(E) * torch.einsum("blhe,bshe->bhls", q.double(), k.double())


@pytest.mark.parametrize("name,E,bf16", [(n, E, False) for n in C.REGIMES for E in C.REGIME_WIDTHS]
                         + [(n, E, True) for n in C.BF16_RESCALED for E in C.REGIME_WIDTHS if ("bf16", E) in C.ROUTES])
def test_regime_inputs_are_what_they_claim(name, E, bf16):
    """bf16: the rows the bf16 route runs where they differ (C.BF16_RESCALED): the same claims hold for them"""
    B, L, S, H = C.REGIME_SHAPE
    q, k, v, go = C.regime_inputs(name, E, bf16)
    assert q.shape == go.shape == (B, L, H, E) and k.shape == v.shape == (B, S, H, E)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (q, k, v, go))
    s = _scores(name, E, bf16)
    top = float(s.abs().max())
    if name == "zero":
        assert top == 0.0 and float(q.abs().max()) == 0.0
    else:
        assert C.SCORE_RANGE[0] <= top <= C.SCORE_RANGE[1], top
    assert S % C.SUB_KEYS != 0 and S % 64 > C.SUB_KEYS, "161 keys: a ragged last tile at both key-tile sizes"
    tiles = [s[..., t:t + C.SUB_KEYS].amax(-1) for t in range(0, S, C.SUB_KEYS)]
    run = torch.stack(tiles, -1).cummax(-1).values                  # running maximum after each 32-key score tile
    if name == "rising":
        assert bool((run[..., 1:] > run[..., :-1]).all()), "a row's maximum stays put in some tile"
    if name == "falling":
        assert bool((run[..., 1:] == run[..., :1]).all()), "a row's maximum is not in the first tile"
    if name == "last":
        assert bool((s.argmax(-1) == S - 1).all())
        assert float(torch.softmax(s, -1)[..., S - 1].min()) > 0.5
    if name == "uniform":
        assert bool((k == k[:, :1]).all())
        p = C.regime_reference(name, E)["probs"]
        assert float((p - 1.0 / S).abs().max()) < 1e-15
        assert float((C.regime_reference(name, E)["out"] - v.double().mean(1, keepdim=True)).abs().max()) < 1e-12
    if name == "tie":
        j1, j2 = C.TIE_KEYS
        rows = list(C.TIE_ROWS)
        assert j1 < C.SUB_KEYS and j2 == S - 1
        assert bool((s[:, :, rows, j1] == s[:, :, rows, j2]).all()), "the two scores are equal term by term"
        half = E // 2
        assert float(q[:, rows][..., half:].abs().max()) == 0.0 and bool((k[:, j1, :, :half] == k[:, j2, :, :half]).all())
        assert bool((k[:, j1, :, half:] == -k[:, j2, :, half:]).all()) and float(k[:, j1, :, half:].abs().min()) > 0
        assert bool((v.abs() == C.TIE_V).all()) and bool((go.abs() == C.TIE_DO).all()) and bool((v[:, j1] == -v[:, j2]).all())
        p = C.regime_reference(name, E)["probs"]
        assert float(p[:, :, rows[0], j1].min()) > 0.499
        dP = torch.einsum("blhd,bshd->bhls", go.double(), v.double())
        dS = p * (dP - (p * dP).sum(-1, keepdim=True))
        hard = 2.0 * E * float(go.abs().max()) * float(v.abs().max())
        assert 0.24 * hard <= float(dS.abs().max()) <= 0.25 * hard, (float(dS.abs().max()), hard)
    if name == "zero":
        assert float(C.regime_reference(name, E)["dk"].abs().max()) == 0.0
        assert float(C.regime_reference(name, E)["dq"].abs().amax((1, 3)).min()) > 0


@pytest.mark.parametrize("E", C.REGIME_WIDTHS)
@pytest.mark.parametrize("name", C.REGIMES)
def test_regime_tolerances_obey_their_condition(name, E):
    """every regime row's fp32 restatement is itself inside the project's bounds, and no tolerance exceeds 4 x the project's bound"""
    for what, (tol, e32, bound) in C.regime_tolerances(name, E).items():
        print(f"{name} E={E} {what}: fp32 restatement {e32:.3g}, tolerance {tol:.3g}, bound {bound:.3g}")
        assert bound == (C.FWD_TOL if what == "out" else C.GRAD_TOL)
        assert tol == max(bound, C.REGIME_MARGIN * e32)
        assert e32 <= bound, (what, e32)
        assert tol <= C.REGIME_MAX_FACTOR * bound, (what, tol)


@pytest.mark.parametrize("E", [E for E in C.REGIME_WIDTHS if ("bf16", E) in C.ROUTES])
@pytest.mark.parametrize("name", C.REGIMES)
def test_bf16_regime_tolerances_obey_the_same_condition(name, E):
    """the bf16 route: max(bound of tests/test_gpu_bf16_parity.py, ATTN_FACTOR x the model's own noise on the case), and no
    tolerance above 4 x that file's bound -- the rows of C.BF16_RESCALED are the ones that had to be rescaled for it"""
    from test_gpu_bf16_parity import ATTN_FACTOR, ATTN_TOL, ATTN_TOL_RMS
    for what, ((tmax, trms), (nmax, nrms)) in C.bf16_regime_tolerances(name, E).items():
        print(f"{name} E={E} {what}: noise {nmax:.3g} / rms {nrms:.3g}, tolerance {tmax:.3g} / rms {trms:.3g}")
        assert tmax == max(ATTN_TOL, ATTN_FACTOR * nmax) and trms == max(ATTN_TOL_RMS, ATTN_FACTOR * nrms)
        assert tmax <= C.REGIME_MAX_FACTOR * ATTN_TOL, (what, tmax / ATTN_TOL)
        assert trms <= C.REGIME_MAX_FACTOR * ATTN_TOL_RMS, (what, trms / ATTN_TOL_RMS)
    if name not in C.BF16_RESCALED:
        assert all(torch.equal(a, b) for a, b in zip(C.regime_inputs(name, E, True), C.regime_inputs(name, E)))


# ----------------------------------------------------------------------------------------------------------------- the wrapper
def test_operand_rule_copies_what_the_kernels_refuse():
    """ops._attn_operand: the kernels take positive batch / sequence strides that are multiples of 4 and a 16-byte aligned base
    (attn_check); everything else is copied, also where torch calls the tensor contiguous already."""
    ops = _ops()
    B, S, H, E = 2, 5, 3, 16
    base = torch.randn(B, S, H, E)
    assert ops._attn_operand(base) is base
    packed = torch.randn(B, S, 3, H, E)
    view = packed[:, :, 1]                                              # a strided view of a packed projection is read in place
    assert ops._attn_operand(view) is view
    for bad in (base[:1].expand(B, -1, -1, -1),                        # stride 0 over the batch: refused by attn_check before
                base[:1, :1].expand(B, S, -1, -1),                     # ... and over the sequence
                base[:1].expand(1, -1, -1, -1).as_strided((1, S, H, E), (0, H * E, E, 1)),   # contiguous to torch, stride 0
                torch.randn(B * S * H * E + 1)[1:].view(B, S, H, E),   # contiguous, base 4 bytes off 16-byte alignment
                torch.randn(B, H, S, E).permute(0, 2, 1, 3),           # head stride not E
                torch.randn(B, S, H, E + 1)[..., :E],                  # sequence stride not a multiple of 4 at the head level
                torch.randn(B, S, H, 2 * E)[..., ::2]):                # element stride 2
        assert not ops._attn_operand_ok(bad)
        got = ops._attn_operand(bad)
        assert ops._attn_operand_ok(got) and got.shape == bad.shape and torch.equal(got, bad)
        assert got.stride() == (S * H * E, H * E, E, 1) or bad.shape[0] == 1
