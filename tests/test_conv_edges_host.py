"""What the convolution / dense GEMM edge table covers and what its tolerance can see -- no GPU (tests/conv_edge_cases.py holds the
table; tests/test_gpu_conv_edges.py runs it).  Checked here: every geometry class of the kernels is reached under every arithmetic
that runs the kernel; the Python restatement of the launch planners agrees with the constants in csrc/ and, where the library is
built, with its host-side queries; the operand regimes are what they claim in float64; every case's tolerance is under its cap;
and a float64 model with one planted defect exceeds the tolerance on at least one case of its regime."""
import os
import re

import pytest
import torch

import conv_edge_cases as C

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-imagery-eeg_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _cases(kind, arith):
    return [c for c in C.CASES if c.kind == kind and arith in C.ariths_of(c)]


# ------------------------------------------------------------------------------------------------------------------ coverage
@pytest.mark.parametrize("arith", C.ARITHS)
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_forward_and_data_gradient_classes_are_reached(kind, arith):
    cs = [c for c in _cases(kind, arith) if c.k <= C.SPLIT_KMAX]
    plans = [(c, C.plan_of(arith, c)) for c in cs]
    narrow = [(c, p) for c, p in plans if not p["wide"]]
    rows, chans, cols = (set(x) for x in zip(*(C.dims(c) for c, _ in narrow)))
    assert {1, 127, 128, 129, 256, 257} <= rows
    assert {4, 64, 124, 128, 132, 256} <= cols
    assert {1, 2, 3, 4, 6, 15, 16, 17, 18, 20, 36} <= chans
    assert {1, 2, 3, 5, 8, 9, 16} <= {c.k for c, _ in narrow}
    assert {1, 2, 4} <= {p["V"] for _, p in narrow}
    assert {"<8", "=8", "8n+r"} <= {C.nwg_class(p["nwg"]) for _, p in narrow}
    assert any(p["remaps"] and p["nwg"] % 8 for _, p in narrow), "a swizzle that moves tiles, with a tail it leaves alone"
    assert any(p["full"] for _, p in narrow) and any(p["ragged_mn"] for _, p in narrow)
    assert any(p["cp"] != C.dims(c)[1] for c, p in narrow) or arith == "f32"              # the padded tail of cp
    assert any(p["K"] % C.KC for _, p in narrow)                                          # fp32: a ragged last chunk
    for V in (4, 2, 1):                                                                   # every epilogue with every V
        if kind == "fwd":
            assert {True, False} <= {c.pro for c, p in narrow if p["V"] == V}, V
        else:
            assert any(p["V"] == V for _, p in narrow), V
        assert {True, False} <= {c.part for c, p in narrow if p["V"] == V}, ("with and without stat_part", V)
    assert {"normal", "pairs", "offset"} <= {c.regime for c in cs}
    if arith == "f16x3":
        assert {"loose", "spike"} <= {c.regime for c in cs}
    if arith == "f32":
        assert any(p["straddle"] for _, p in narrow), "a tile that holds rows of two samples"
        assert any(c.k == 17 for c in _cases(kind, arith))
    else:
        assert all(arith in C.refused_ariths(c) for c in C.CASES if c.k == 17)


@pytest.mark.parametrize("arith", C.SPLIT_ARITHS)
def test_wide_tile_classes_are_reached(arith):
    wide = [(c, p) for c in _cases("fwd", arith) for p in [C.plan_of(arith, c)] if p["wide"]]
    assert {1, 127, 128, 129} <= {C.dims(c)[0] for c, _ in wide}
    # (not counted: the `coarse` cases, whose operands are exact in one plane -- they show plane 0 and the grid, nothing else)
    live = [(c, p) for c, p in wide if c.regime != "coarse"]
    assert all(C.bound(c, arith).e_model != 0 for c, _ in live) or arith == "bf16"
    assert {256, 512} <= {c.Co for c, _ in live} and {4, 20, 256} <= {c.Ci for c, _ in live}
    assert any(c.Co == 512 and c.regime == "normal" and p["mtiles"] == 1 for c, p in live)
    assert {4, 20} <= {c.Ci for c, _ in wide if c.Co == 512}
    assert {"<8", "=8", "8n+r"} <= {C.nwg_class(p["nwg"]) for _, p in wide}
    assert any(p["remaps"] and p["nwg"] % 8 for _, p in wide)
    # the rule itself: each condition that sends a k = 1, N % 256 == 0 layer back to the 128 x 128 kernel
    assert C.nt_plan(arith, 1, 128, 4, 256, 1, part=False)["wide"]
    for kw in (dict(B=2), dict(C=6), dict(N=384), dict(k=2), dict(pro=True), dict(part=True), dict(epi="mask")):
        a = dict(B=1, rows=128, C=4, N=256, k=1, pro=False, epi="bias", part=False)
        a.update(kw)
        assert not C.nt_plan(arith, **a)["wide"], kw


def test_gelu_and_plain_epilogues_are_reached():
    gelu = [c for c in C.CASES if c.kind == "gelu"]
    assert {1, 127, 128, 129} <= {c.Tin for c in gelu} and all(C.ariths_of(c) == ("f16x3",) for c in gelu)
    assert all(C.plan_of("f16x3", c)["wide"] and c.Ci % 256 == 0 and c.Co % 4 == 0 for c in gelu)
    for arith in C.ARITHS:
        plain = [c for c in _cases("dgrad_input", arith) if c.k <= C.SPLIT_KMAX]
        assert plain and all(c.Ci % 4 and c.Co % 4 == 0 for c in plain)
        assert {1, 2} <= {C.vec_width(c.Ci) for c in plain}, "odd and even ragged output columns"


@pytest.mark.parametrize("arith", C.SPLIT_ARITHS)
def test_multi_tap_weight_gradient_classes_are_reached(arith):
    cs = [c for c in _cases("wgrad", arith) if c.k in C.WGRAD_RU]
    plans = [(c, C.wgrad_x6_plan(c.B, c.Tin, c.Ci, c.Co, c.k)) for c in cs]
    for k, ru in C.WGRAD_RU.items():
        assert {1, ru - 1, ru, ru + 1} <= {c.Tin - k + 1 for c in cs if c.k == k}, k
        assert {True, False} <= {c.pro for c in cs if c.k == k}
    assert {4, 60, 64, 68} <= {c.Co for c in cs} and {1, 2, 3, 63, 64, 66} <= {c.Ci for c in cs}
    assert any(p["nsplit"] == 1 for _, p in plans)
    assert any(p["nsplit"] > 1 and p["ragged_last"] and not p["empty"] for _, p in plans)
    assert any(c.defer for c in cs) and {"normal", "offset", "pairs"} <= {c.regime for c in cs}
    if arith == "f16x3":
        assert {"loose", "spike"} <= {c.regime for c in cs}
    capped = C.find(*C.CAPPED["bf16x6"])
    p = C.wgrad_x6_plan(capped.B, capped.Tin, capped.Ci, capped.Co, capped.k)
    assert (p["nunits"], p["tiles"], p["nsplit"], p["per"], p["empty"]) == (4100, 2, 256, 17, 14)
    assert p["nsplit"] == C.cdiv(C.WGRAD_X6_TARGET, p["tiles"]) < C.cdiv(p["nunits"], C.WGRAD_X6_MIN_UNITS), "capped by the tiles"


@pytest.mark.parametrize("arith", C.ARITHS)
def test_dense_weight_gradient_classes_are_reached(arith):
    cs = _cases("wgrad_k1", arith)
    assert {1, 15, 16, 17, 511, 512, 513} <= {c.Tin for c in cs}
    assert {4, 124, 128, 132} <= {c.Co for c in cs} and {4, 124, 128, 132} <= {c.Ci for c in cs}
    assert {True, False} <= {c.db for c in cs} and {"normal", "pairs", "offset"} <= {c.regime for c in cs}
    plans = [C.wgrad_k1_plan(c.Tin, c.Ci, c.Co) for c in cs]
    assert any(p["nsplit"] % 8 and p["nsplit"] > 1 and p["grid"] > p["tiles"] * p["nsplit"] for p in plans)
    capped = C.find(*C.CAPPED["k1"])
    p = C.wgrad_k1_plan(capped.Tin, capped.Ci, capped.Co)
    assert (p["nunits"], p["tiles"], p["nsplit"], p["per"], p["empty"]) == (16400, 1, 512, 33, 15)


def test_fp32_weight_gradient_classes_are_reached():
    cs = _cases("wgrad", "f32")
    assert all(any(c.k == k and c.Ci % 2 for c in cs) for k in (4, 7, 9))
    assert any(c.k * c.Ci > 128 and (c.k * c.Ci) % 128 for c in cs), "k * Ci ragged against the second 128-column tile"
    assert {1, 2, 4} <= {C.vec_width(c.Ci) for c in cs} and any(c.k == 17 for c in cs)
    capped = C.find(*C.CAPPED["f32"])
    p = C.wgrad_f32_plan(capped.B, capped.Tin, capped.Ci, capped.Co, capped.k)
    assert (p["nsplit"], p["rows_per"], p["empty"]) == (1024, 144, 112)
    sizes = [max(t.numel() for t in C.inputs(c).values() if torch.is_tensor(t)) for c in C.CASES]
    top3 = sorted(range(len(sizes)), key=lambda i: -sizes[i])[:3]
    assert {(C.CASES[i].kind, C.CASES[i].name) for i in top3} == set(C.CAPPED.values()), "the tile-capped cases are the largest"
    assert 4 * max(sizes) < 40e6


# ------------------------------------------------------------------------------------------ the restatement against the sources
def _body(src, signature):
    """the text of the function whose definition starts with `signature`, up to the first line that is just `}`"""
    m = re.search(re.escape(signature) + r".*?\n}\n", src, re.S)
    assert m, signature
    return m.group(0)


def _ints(pattern, text):
    m = re.search(pattern, text)
    assert m, (pattern, text[:200])
    return tuple(int(x) for x in m.groups())


def test_restatement_agrees_with_the_kernel_sources():
    h, x6, f32 = _src("ign_clconv.h"), _src("ign_clconv_x6.hip"), _src("ign_clconv_f32.hip")
    assert _ints(r"constexpr int TM = (\d+), TN = (\d+), KC = (\d+);", h) == (C.TM, C.TN, C.KC)
    assert _ints(r"constexpr int X6T_SPAN = TM \+ (\d+);", x6)[0] + C.TM == C.X6T_SPAN == C.TM + C.SPLIT_KMAX - 1
    assert len(re.findall(r"if \((?:x6 && )?k > (\d+)\)", f32)) == 2 and set(re.findall(r"if \((?:x6 && )?k > (\d+)\)", f32)) == {str(C.SPLIT_KMAX)}
    assert "inline int ign_vec_width(int c) { return (c % 4 == 0) ? 4 : (c % 2 == 0) ? 2 : 1; }" in h
    # rows per unit
    ru = _body(x6, "static int wgrad_x6_rows_per_unit(int k)")
    table = {}
    for ka, kb, r in re.findall(r"\(k == (\d+) \|\| k == (\d+)\) \? (\d+)", ru):
        table[int(ka)] = table[int(kb)] = int(r)
    assert table == C.WGRAD_RU
    assert x6.count("launch_wgrad_x6<8, 1, NP>") == 1 and x6.count("launch_wgrad_x6<5, 1, NP>") == 1          # NR = ru / 16
    assert x6.count("launch_wgrad_x6<3, 2, NP>") == 1 and x6.count("launch_wgrad_x6<2, 2, NP>") == 1
    assert "constexpr int RU = 16 * NR;" in x6
    # split planners
    s = _body(x6, "static int wgrad_x6_splits(int nunits, int tiles)")
    assert _ints(r"int s = \((\d+) \+ tiles - 1\) / tiles;", s) == (C.WGRAD_X6_TARGET,)
    assert _ints(r"max_s = \(nunits \+ (\d+)\) / (\d+);", s) == (C.WGRAD_X6_MIN_UNITS - 1, C.WGRAD_X6_MIN_UNITS)
    s = _body(x6, "static int wgrad_x6_k1_splits(")
    assert _ints(r"\*nunits = \(int\)\(\(M \+ (\d+)\) / (\d+)\);", s) == (C.WGRAD_K1_UNIT - 1, C.WGRAD_K1_UNIT)
    assert _ints(r"int s = \((\d+) \+ \*tiles - 1\) / \*tiles;", s) == (C.WGRAD_K1_TARGET,)
    assert _ints(r"max_s = \(\*nunits \+ (\d+)\) / (\d+);", s) == (C.WGRAD_K1_MIN_UNITS - 1, C.WGRAD_K1_MIN_UNITS)
    assert "((Co + 127) / 128) * ((Ci + 127) / 128)" in s and "(w.nsplit + 7) / 8 * 8" in x6
    s = _body(f32, "static int wgrad_splits(long long M, int tiles)")
    assert _ints(r"s = \((\d+) \+ tiles - 1\) / tiles;", s) == (C.WGRAD_F32_TARGET,)
    assert _ints(r"max_s = \(M \+ (\d+) \* KC - 1\) / \((\d+) \* KC\);", s) == (C.WGRAD_F32_MIN_CHUNKS,) * 2
    # what the kernels derive from the plan
    assert "const int rows_per = ((a.M + a.nsplit - 1) / a.nsplit + KC - 1) / KC * KC;" in f32
    assert x6.count("const int per = (a.nunits + a.nsplit - 1) / a.nsplit;") == 2
    assert x6.count("const int per = nwg / 8;") == 2 and f32.count("const int per = nwg / 8;") == 1
    assert x6.count("if (lid < per * 8) lid = (lid & 7) * per + (lid >> 3);") == 2
    assert "const int tiles = ((Co + 63) / 64) * a.citiles;" in x6 and "a.citiles = (Ci + 63) / 64;" in x6
    assert "c.tps = (Tout + TM - 1) / TM;" in f32 and "c.tps = (Tin + TM - 1) / TM;" in f32 and f32.count("c.g.mtiles = B * c.tps;") == 2
    assert "a.k == 1 && a.g.N % 256 == 0 && V == 4 && !pro && epi == EPI_BIAS_STATS && !a.g.part &&" in x6


def test_the_swizzle_is_a_permutation_of_the_tiles():
    for nwg in (1, 7, 8, 9, 12, 16, 18, 22, 30, 64, 67):
        per = nwg // 8
        lids = sorted((b & 7) * per + (b >> 3) if b < per * 8 else b for b in range(nwg))
        assert lids == list(range(nwg)), nwg


def _lib_or_skip():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so is not built")
    return _lib.lib()


def test_restatement_agrees_with_the_library():
    L = _lib_or_skip()
    for c in range(1, 300):
        assert L.ign_clconv_kpad(c) == C.kpad(c)
    for c in C.CASES:
        B, Tin, Ci, Co, k = c.B, c.Tin, c.Ci, c.Co, c.k
        assert L.ign_clconv_x3_elems(Co, Ci, k) == C.x3_elems(Co, Ci, k) and L.ign_clconv_x3_elems(Ci, Co, k) == C.x3_elems(Ci, Co, k)
        if c.kind in ("fwd", "dgrad", "dgrad_input", "gelu"):
            rows, ch, n = C.dims(c)
            assert L.ign_clconv_x6_mtiles(B, rows) == C.nt_plan("bf16x6", B, rows, ch, n, k)["mtiles"], c
            assert L.ign_clconv_mtiles(B * rows) == C.nt_plan("f32", B, rows, ch, n, k)["mtiles"], c
            continue
        f = C.wgrad_f32_plan(B, Tin, Ci, Co, k)
        assert L.ign_clconv_wgrad_workspace_bytes(B, Tin, Ci, Co, k) == 4 * f["ws_floats"], c
        if k == 1:
            assert L.ign_clconv_wgrad_x6_workspace_bytes(B, Tin, Ci, Co, k) == 4 * C.wgrad_k1_plan(B * Tin, Ci, Co)["ws_floats"], c
        elif k in C.WGRAD_RU:
            p = C.wgrad_x6_plan(B, Tin, Ci, Co, k)
            assert L.ign_clconv_wgrad_x6_nsplit(B, Tin, Ci, Co, k) == p["nsplit"], c
            assert L.ign_clconv_wgrad_x6_workspace_bytes(B, Tin, Ci, Co, k) == 4 * p["ws_floats"], c
        else:
            assert L.ign_clconv_wgrad_x6_nsplit(B, Tin, Ci, Co, k) == 0 and L.ign_clconv_wgrad_x6_workspace_bytes(B, Tin, Ci, Co, k) == 0


# ------------------------------------------------------------------------------------------------------------------- regimes
def test_regimes_are_what_they_claim_in_float64():
    seen = set()
    for c in C.CASES:
        d = C.inputs(c)
        a, b = d["a"].double(), d["b"].double()
        seen.add(c.regime)
        wgrad = c.kind in ("wgrad", "wgrad_k1")
        if c.regime == "pairs":
            # the leading products of a pair cancel: the exact result is 2^-9 of the conditioning, i.e. it lives in the cross terms
            bd = C.bound(c, "f32")
            assert float((bd.exact.abs() / bd.cond).max()) < 2.0 ** -9, c
            dim = 2 if not wgrad else 1 if c.kind == "wgrad_k1" else 0
            even, odd = a.index_select(dim, torch.arange(0, a.shape[dim] - 1, 2)), a.index_select(dim, torch.arange(1, a.shape[dim], 2))
            r = (odd / even - 1) * 2 ** 9
            assert float(r.abs().max()) <= 1 + 2.0 ** -14 and float(r.abs().mean()) > 0.3, c
        if c.regime == "offset":
            assert float((a - 1000).abs().max()) < 7 and float((a - 1000).std()) > 0.9, c
            sums = b.sum((0, 1)) if wgrad else b.sum((1, 2)) if c.kind == "fwd" else b.sum((0, 2))
            scale = b.abs().sum((0, 1)) if wgrad else b.abs().sum((1, 2)) if c.kind == "fwd" else b.abs().sum((0, 2))
            assert float((sums.abs() / scale).max()) < 1e-6, c                # every filter sums to zero (to fp32 rounding of its taps)
        if c.regime == "coarse":
            assert bool(((a * 64).round() == a * 64).all()) and bool(((b * 64).round() == b * 64).all()) and float(a.abs().max()) <= 1
        if c.regime in C.F16_ONLY_REGIMES:
            s = C.pow2_scale(d["bound_a"])
            top = float(a.abs().max()) * s
            assert 2.0 ** 13 <= d["bound_a"] * s < 2.0 ** 14
            if c.regime == "loose":
                assert 2.0 ** 3 <= top < 2.0 ** 4, "ten bits of the leading plane's range are not used"
            else:
                rest = a.abs().flatten().sort().values[-2]
                assert 2.0 ** 13 <= top < 2.0 ** 14 and float(a.abs().max() / rest) >= 2.0 ** 8, c
        elif c.kind != "gelu":
            assert d["bound_a"] == float(d["a"].abs().max()) and d["bound_b"] == float(d["b"].abs().max()), "the bound given exactly"
    assert seen == set(C.REGIMES)
    for bnd in (1.0, 0.9999, 2.0, 3e6, 1e-6, 65504.0):
        assert 2.0 ** 13 <= bnd * C.pow2_scale(bnd) < 2.0 ** 14
    assert C.pow2_scale(0.0) == C.pow2_scale(float("inf")) == 1.0 and C.pow2_scale(1e-30) == 2.0 ** 60


# ----------------------------------------------------------------------------------------------------------------- tolerance
@pytest.mark.parametrize("kind", ["fwd", "dgrad", "dgrad_input", "gelu", "wgrad", "wgrad_k1"])
def test_tolerance_is_under_its_cap_on_every_case(kind):
    for c in C.CASES:
        if c.kind != kind:
            continue
        for arith in C.ariths_of(c):
            bd = C.bound(c, arith)
            print(f"{kind} {c.name} {arith}: E_model {bd.e_model:.3f} E_acc {bd.e_acc:.3f} tol {bd.tol:.3f} cap {bd.cap:.0f}")
            assert bd.tol <= bd.cap, (c, arith, bd.e_model, bd.e_acc)
            assert bd.tol >= C.TOL_FLOOR and (bd.e_model == 0.0) == (arith in ("f32", "bf16") or c.regime == "coarse")
            assert bool((bd.exact[bd.cond == 0] == 0).all()), "no scale (operands the ReLU prologue zeroed): the element is exactly 0"


def _worst(what, arith, cases):
    return max((C.defect_units(c, arith, what) / C.bound(c, arith).tol, c.name) for c in cases)


def test_the_tolerance_sees_each_planted_defect():
    nt = [c for c in C.CASES if c.kind in ("fwd", "dgrad") and c.k <= C.SPLIT_KMAX]
    for regime in ("normal", "pairs", "offset"):
        cs = [c for c in nt if c.regime == regime]
        for what, arith in (("a1*b1 dropped", "bf16x6"), ("h1*h0 dropped", "f16x3")):
            ratio, name = _worst(what, arith, cs)
            print(f"{what} [{regime}]: {ratio:.1f} x tolerance at {name}")
            assert ratio > 1, (what, regime)
        shifted = [c for c in cs if c.k > 1]
        for arith in C.ARITHS:
            ratio, name = _worst("one tap shifted by a row", arith, shifted)
            print(f"one tap shifted [{regime}, {arith}]: {ratio:.1f} x tolerance at {name}")
            assert ratio > 1, (arith, regime)
            padded = [c for c in cs if C.dims(c)[1] % 16]
            ratio, name = _worst("padded channels read the neighbour", arith, padded)
            print(f"padded channels [{regime}, {arith}]: {ratio:.1f} x tolerance at {name}")
            assert ratio > 1, (arith, regime)
    for arith, key in (("bf16x6", "bf16x6"), ("f16x3", "bf16x6"), ("bf16", "bf16x6"), ("bf16x6", "k1"), ("f16x3", "k1"), ("bf16", "k1"),
                       ("f32", "f32")):
        c = C.find(*C.CAPPED[key])
        ratio = C.defect_units(c, arith, "empty split returns stale data") / C.bound(c, arith).tol
        print(f"stale empty split [{arith}, {c.name}]: {ratio:.1f} x tolerance")
        assert ratio > 1, (arith, key)
