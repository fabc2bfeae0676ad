"""Case tables, launch geometry and bounds of the convolution / dense GEMM edge tests (csrc/ign_clconv_f32.hip, ign_clconv_x6.hip).

Three things live here, shared by tests/test_conv_edges_host.py (no GPU), tests/test_gpu_conv_edges.py and tests/diag_conv_edges.py:

  * a pure-Python restatement of the launch planners (`nt_plan`, `wgrad_x6_plan`, `wgrad_k1_plan`, `wgrad_f32_plan`): from
    (B, Tin, Ci, Co, k) the staging width V, padded channels, tiles, steps, workgroup count and swizzle, the wide-tile rule, and the
    split planners of the three weight-gradient kernels with their empty trailing splits;
  * the case table (`CASES`), chosen from those branch points, and the operand regimes;
  * the float64 reference, the float64 emulation of each arithmetic's split, and the tolerance rule.

Every kernel here is a bilinear product of two operands (activation x weight, gradient x weight, gradient x activation); `product`
states it once per kind, and the reference, the conditioning `sum |a||b|`, the split emulations and the planted defects are all that
one function applied to different operand planes.

Tolerance (DESIGN.md 4.6c', "What covers the GEMM edges"): the unit is u * cond per element, u = 2^-24, cond = product(|A|, |W|) + |bias| with
A the operand after the prologue.  A case is held to E_model + max(1, 4 * E_acc) units: E_model = the error of the float64
emulation of the arithmetic's split and dropped terms against exact float64 (0 for f32, 0 by construction for bf16, whose
reference is the product of the rounded operands), E_acc = the error of torch's float32 evaluation of the same operands on the CPU.
No case may exceed 16 units or K + 8 (K = reduction length); tests/test_conv_edges_host.py checks that on every case."""
import functools
import math
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

U = 2.0 ** -24
TM = TN = 128
KC = 16
X6T_SPAN = TM + 15
SPLIT_KMAX = 16                                     # taps the split kernels stage (X6T_SPAN - TM + 1)
ARITHS = ("f32", "bf16x6", "f16x3", "bf16")
SPLIT_ARITHS = ARITHS[1:]
WGRAD_RU = {8: 16, 5: 16, 3: 32, 2: 32}             # rows per unit of clconv_wgrad_x6_kernel
WGRAD_X6_TARGET, WGRAD_X6_MIN_UNITS = 512, 16       # wgrad_x6_splits
WGRAD_K1_TARGET, WGRAD_K1_MIN_UNITS, WGRAD_K1_UNIT = 512, 32, 16    # wgrad_x6_k1_splits
WGRAD_F32_TARGET, WGRAD_F32_MIN_CHUNKS = 1024, 8    # wgrad_splits
TOL_FLOOR, TOL_FACTOR, TOL_CAP = 1.0, 4.0, 16.0
IGN_E_UNSUP = -1002


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------ launch geometry
def vec_width(c):
    return 4 if c % 4 == 0 else 2 if c % 2 == 0 else 1


def kpad(c):
    return cdiv(c, 16) * 16


def x3_elems(rows, chans, k):
    return 3 * cdiv(rows, TN) * TN * k * kpad(chans)


def wide_rule(split, B, C, N, k, pro, epi, part):
    """ign_clconv_launch_x6t: the 128 x 256 tile kernel (a Linear layer with wide outputs); the GELU-gradient epilogue runs only there"""
    if not split:
        return False
    if epi == "gelu":
        return True
    return k == 1 and N % 256 == 0 and vec_width(C) == 4 and not pro and epi == "bias" and not part and B == 1


def nt_plan(arith, B, rows, C, N, k, pro=False, epi="bias", part=True):
    """Forward (rows = Tout, C = Ci, N = Co) or data gradient (rows = Tin, C = Co, N = Ci).  The split kernels tile each sample on
    its own (tps tiles per sample); the fp32 kernel tiles the B * rows matrix, so a tile can straddle samples."""
    split = arith != "f32"
    M = B * rows
    if split:
        tps, cp = cdiv(rows, TM), kpad(C)
        mtiles, steps = B * tps, cp // KC * k
        tiles = [(b * rows + t * TM, b * rows + min(rows, t * TM + TM)) for b in range(B) for t in range(tps)]
    else:
        tps, cp = None, C
        mtiles, steps = cdiv(M, TM), cdiv(k * C, KC)
        tiles = [(m * TM, min(M, m * TM + TM)) for m in range(mtiles)]
    wide = wide_rule(split, B, C, N, k, pro, epi, part)
    ntiles = N // 256 if wide else cdiv(N, TN)
    tn = 256 if wide else TN
    nwg = mtiles * ntiles
    per = nwg // 8
    full = any(e - s == TM for s, e in tiles) and N >= tn
    ragged_mn = any(e - s < TM for s, e in tiles) and N % tn != 0
    straddle = (not split) and any(s // rows != (e - 1) // rows for s, e in tiles)
    return dict(V=vec_width(C), cp=cp, tps=tps, mtiles=mtiles, ntiles=ntiles, steps=steps, nwg=nwg, per=per, remaps=per >= 2,
                wide=wide, tiles=tiles, full=full, ragged_mn=ragged_mn, straddle=straddle, K=k * C,
                kernel=("clconv_x6w_kernel" if wide else "clconv_x6t_kernel") if split else "clconv_nt_kernel")


def nwg_class(nwg):
    return "<8" if nwg < 8 else "=8" if nwg == 8 else "8n+r" if nwg % 8 else "8n"


def _splits(nunits, tiles, target, min_units):
    return max(1, min(cdiv(target, tiles), cdiv(nunits, min_units)))


def wgrad_x6_plan(B, Tin, Ci, Co, k):
    """clconv_wgrad_x6_kernel (k in 8, 5, 3, 2): units of ru output rows that never straddle a sample, split over unit ranges"""
    Tout, ru = Tin - k + 1, WGRAD_RU[k]
    cps = cdiv(Tout, ru)
    nunits, tiles = B * cps, cdiv(Co, 64) * cdiv(Ci, 64)
    nsplit = _splits(nunits, tiles, WGRAD_X6_TARGET, WGRAD_X6_MIN_UNITS)
    per = cdiv(nunits, nsplit)
    used = cdiv(nunits, per)
    return dict(ru=ru, cps=cps, nunits=nunits, tiles=tiles, nsplit=nsplit, per=per, empty=nsplit - used,
                ragged_last=nunits - (used - 1) * per != per, V=vec_width(Ci), ws_floats=nsplit * Co * k * Ci, part_floats=nsplit * Co * k * Ci,
                K=B * Tout, kernel="clconv_wgrad_x6_kernel")


def wgrad_k1_plan(M, Ci, Co):
    """clconv_wgrad_x6_k1_kernel: units of 16 rows; the grid is tiles x (splits rounded up to the 8 XCDs)"""
    nunits, tiles = cdiv(M, WGRAD_K1_UNIT), cdiv(Co, 128) * cdiv(Ci, 128)
    nsplit = _splits(nunits, tiles, WGRAD_K1_TARGET, WGRAD_K1_MIN_UNITS)
    per = cdiv(nunits, nsplit)
    used = cdiv(nunits, per)
    return dict(nunits=nunits, tiles=tiles, nsplit=nsplit, per=per, empty=nsplit - used, grid=tiles * cdiv(nsplit, 8) * 8,
                ws_floats=nsplit * Co * (Ci + 1), part_floats=nsplit * Co * Ci, K=M, kernel="clconv_wgrad_x6_k1_kernel")


def wgrad_f32_plan(B, Tin, Ci, Co, k):
    """clconv_tn_kernel: 128 x 128 tiles of (Co, k * Ci), split over row ranges rounded up to the 16-row chunk"""
    M = B * (Tin - k + 1)
    tiles = cdiv(Co, 128) * cdiv(k * Ci, 128)
    nsplit = max(1, min(cdiv(WGRAD_F32_TARGET, tiles), cdiv(M, WGRAD_F32_MIN_CHUNKS * KC)))
    rows_per = cdiv(cdiv(M, nsplit), KC) * KC
    used = cdiv(M, rows_per)
    return dict(tiles=tiles, nsplit=nsplit, rows_per=rows_per, empty=nsplit - used, V=vec_width(Ci), ws_floats=nsplit * Co * k * Ci,
                part_floats=nsplit * Co * k * Ci, K=M, kernel="clconv_tn_kernel")


def wgrad_plan(arith, case):
    """the planner that runs for this case under this arithmetic"""
    if arith == "f32":
        return wgrad_f32_plan(case.B, case.Tin, case.Ci, case.Co, case.k)
    if case.k == 1:
        return wgrad_k1_plan(case.B * case.Tin, case.Ci, case.Co)
    return wgrad_x6_plan(case.B, case.Tin, case.Ci, case.Co, case.k)


# ------------------------------------------------------------------------------------------------------------------ the cases
# kind: fwd | dgrad | dgrad_input | gelu | wgrad | wgrad_k1 (the Linear entry points, with db).  regime: see `REGIMES`.
Case = namedtuple("Case", "kind name B Tin Ci Co k pro part regime db defer")
# loose, spike: f16x3 only (the bound 2^10 too loose / one element 2^10 above the rest).  coarse: operands n / 64, |n| <= 64 -- every
# product is exact in every arithmetic, for the cases that are about the grid (hundreds of thousands of outputs, where the maxima of
# the reference-side errors of N(0, 1) operands alone leave the cap); what remains is the order of the additions
REGIMES = ("normal", "pairs", "offset", "loose", "spike", "coarse")
F16_ONLY_REGIMES = ("loose", "spike")


def _case(kind, B, Tin, Ci, Co, k, pro=False, part=True, regime="normal", db=False, defer=False, tag=""):
    name = f"B{B}-T{Tin}-Ci{Ci}-Co{Co}-k{k}" + ("-pro" if pro else "") + ("" if part or kind not in ("fwd", "dgrad") else "-nopart") \
        + ("-db" if db else "") + ("-defer" if defer else "") + (f"-{regime}" if regime != "normal" else "") + (f"-{tag}" if tag else "")
    return Case(kind, name, B, Tin, Ci, Co, k, pro, part, regime, db, defer)


# GEMM geometries (B, rows per sample, reduction channels C, output columns N, taps k, prologue, partials): together they reach rows
# 1 / 127 / 128 / 129 / 256 / 257, columns 4 / 64 / 124 / 128 / 132 / 256, channels 1 / 2 / 3 / 4 / 6 / 15 / 16 / 17 / 18 / 20 / 36,
# taps 1 / 2 / 3 / 5 / 8 / 9 / 16, every V with and without the prologue, workgroup counts < 8, = 8 and 8n + r under both tilings.
_GEOMS = [
    (1, 1, 1, 4, 1, False, False),          # one row, one channel, one tap: V = 1, no partials
    (2, 127, 2, 4, 2, False, True),         # V = 2; K = 4
    (1, 128, 3, 124, 3, True, True),        # ragged columns, V = 1 with the prologue
    (1, 129, 4, 128, 5, True, True),        # one row into the second tile, V = 4 with the prologue
    (1, 256, 6, 132, 8, True, True),        # two full m-tiles, four columns into the second n-tile, V = 2 with the prologue
    (3, 257, 15, 4, 9, False, True),        # last chunk holds 15 of 16 channels; 9 workgroups (f32: 7)
    (8, 128, 16, 4, 16, False, True),       # exactly one chunk, 16 taps, 8 workgroups under both tilings
    (9, 257, 17, 4, 1, True, True),         # one channel into the second chunk; 27 workgroups (f32: 19): the swizzle remaps
    (1, 127, 18, 256, 2, True, False),      # two n-tiles; V = 2 without partials
    (1, 129, 20, 124, 3, False, False),     # ragged m x ragged n in tile (1, 0), no partials
    (1, 128, 36, 128, 5, True, True),       # exactly one full tile; 36 channels pad to 48
    (5, 50, 6, 64, 3, False, True),         # fp32 kernel: tile 0 holds samples 0, 1 and part of 2
]
_REGIME_GEOMS = [(2, 127, 2, 4, 2), (1, 129, 20, 124, 3), (1, 128, 36, 128, 5)]                  # pairs, offset
# loose, spike (f16x3): short reductions and few columns -- after the spike enters an fp32 accumulator every later addition rounds at
# ITS scale, in the float32 reference as in the kernels, so the reference-side tolerance of a long reduction leaves the cap
_F16_GEOMS = [(2, 127, 2, 4, 2), (1, 129, 4, 4, 5), (1, 128, 3, 4, 3)]
# wide-tile kernel (B = 1, k = 1, N % 256 == 0, C % 4 == 0, no prologue, no partials): (M, C, N); 1 / 2 / 2 / 2 / 8 / 18 workgroups
_WIDE = [(1, 4, 256, "normal"), (127, 20, 256, "normal"), (128, 256, 256, "normal"), (129, 20, 256, "normal"),
         (1, 20, 512, "normal"), (5, 256, 512, "normal"),        # the second 256-column tile with every plane of both operands live
         (129, 4, 512, "coarse"), (512, 4, 512, "coarse"), (1100, 20, 512, "coarse")]
_GELU = [(1, 4, 256), (127, 20, 256), (128, 256, 256), (129, 20, 256)]                     # (M, Co, Ci) of ign_linear_dgrad_gelu_h3
_DGRAD_INPUT = [(2, 127, 1, 4, 3), (1, 129, 6, 20, 8), (1, 257, 122, 16, 5)]              # (B, Tin, Ci, Co, k): Ci not a multiple of 4
# multi-tap weight gradient (B, Tout, Ci, Co, k, prologue, deferred): per k the rows 1, ru - 1, ru, ru + 1
_WGRAD = [
    (1, 1, 1, 4, 8, False, False), (2, 15, 2, 60, 8, True, False), (19, 16, 3, 64, 8, False, False), (3, 17, 63, 68, 8, True, False),
    (1, 1, 64, 4, 5, True, False), (2, 15, 66, 60, 5, False, False), (1, 16, 1, 64, 5, True, True), (2, 17, 2, 68, 5, False, False),
    (1, 1, 3, 60, 3, False, False), (2, 31, 63, 64, 3, True, False), (1, 32, 64, 68, 3, False, False), (3, 33, 66, 4, 3, True, False),
    (1, 1, 66, 4, 2, True, False), (1, 31, 1, 68, 2, False, False), (20, 32, 2, 60, 2, True, False), (2, 33, 3, 64, 2, False, True),
]
_WGRAD_CAPPED = (2050, 33, 4, 128, 3)              # 4100 units, 2 tiles: 256 splits of 17 units, the last 14 empty
_WGRAD_K1 = [(1, 4, 4, True), (15, 124, 128, False), (16, 128, 132, True), (17, 132, 124, False), (511, 4, 132, True),
             (512, 132, 4, False), (513, 128, 128, True)]                                  # (M, Ci, Co, db)
_WGRAD_K1_CAPPED = (262400, 4, 4)                  # 16400 units, 1 tile: 512 splits of 33 units, the last 15 empty
_WGRAD_F32 = [(2, 20, 3, 4, 4, False), (3, 33, 5, 64, 7, True), (2, 50, 15, 132, 9, False)]      # (B, Tout, Ci, Co, k, prologue)
_WGRAD_F32_CAPPED = (1, 131200, 1, 4, 2)           # 1024 splits of 144 rows, the last 112 empty
_K17 = (2, 20, 3, 4, 17)                           # (B, rows, C, N, k): the fp32 kernels run 17 taps, the split entry points refuse


def _build_cases():
    cs = []
    for B, R, C, N, k, pro, part in _GEOMS:
        cs.append(_case("fwd", B, R + k - 1, C, N, k, pro, part))
        cs.append(_case("dgrad", B, R, N, C, k, False, part))
    for geoms, regimes in ((_REGIME_GEOMS, ("pairs", "offset")), (_F16_GEOMS, F16_ONLY_REGIMES)):
      for B, R, C, N, k in geoms:
        for regime in regimes:
            cs.append(_case("fwd", B, R + k - 1, C, N, k, regime=regime))
            cs.append(_case("dgrad", B, R, N, C, k, regime=regime))
    for M, C, N, regime in _WIDE:
        cs.append(_case("fwd", 1, M, C, N, 1, False, False, regime=regime, tag="wide"))
    cs.append(_case("fwd", 1, 128, 256, 256, 1, False, False, regime="pairs", tag="wide"))
    cs.append(_case("fwd", 1, 129, 4, 512, 1, False, False, regime="loose", tag="wide"))
    for M, Co, Ci in _GELU:
        cs.append(_case("gelu", 1, M, Ci, Co, 1))
    for B, Tin, Ci, Co, k in _DGRAD_INPUT:
        cs.append(_case("dgrad_input", B, Tin, Ci, Co, k))
    for B, Tout, Ci, Co, k, pro, defer in _WGRAD:
        cs.append(_case("wgrad", B, Tout + k - 1, Ci, Co, k, pro, defer=defer))
    cs.append(_case("wgrad", 3, 33 + 2, 66, 4, 3, regime="offset"))
    cs.append(_case("wgrad", 4, 17 + 7, 3, 64, 8, regime="pairs"))
    cs.append(_case("wgrad", 2, 33 + 2, 66, 4, 3, regime="pairs"))
    cs.append(_case("wgrad", 19, 16 + 7, 3, 64, 8, regime="loose"))
    cs.append(_case("wgrad", 1, 8 + 7, 3, 4, 8, regime="spike"))          # (8 rows, 96 outputs: see _F16_GEOMS)
    B, Tout, Ci, Co, k = _WGRAD_CAPPED
    cs.append(_case("wgrad", B, Tout + k - 1, Ci, Co, k, tag="capped"))
    for M, Ci, Co, db in _WGRAD_K1:
        cs.append(_case("wgrad_k1", 1, M, Ci, Co, 1, db=db))
    for regime in ("pairs", "offset", "loose", "spike"):
        cs.append(_case("wgrad_k1", 1, 512, 132, 4, 1, regime=regime))
    M, Ci, Co = _WGRAD_K1_CAPPED
    cs.append(_case("wgrad_k1", 1, M, Ci, Co, 1, db=True, tag="capped"))
    for B, Tout, Ci, Co, k, pro in _WGRAD_F32:
        cs.append(_case("wgrad", B, Tout + k - 1, Ci, Co, k, pro))
    B, Tout, Ci, Co, k = _WGRAD_F32_CAPPED
    cs.append(_case("wgrad", B, Tout + k - 1, Ci, Co, k, tag="capped"))
    B, R, C, N, k = _K17
    cs += [_case("fwd", B, R + k - 1, C, N, k), _case("dgrad", B, R, N, C, k), _case("wgrad", B, R + k - 1, C, N, k),
           _case("dgrad_input", B, R, 3, 4, k)]
    names = [(c.kind, c.name) for c in cs]
    assert len(set(names)) == len(names), "duplicate case"
    return cs


CASES = _build_cases()
CAPPED = {"bf16x6": ("wgrad", _case("wgrad", 2050, 35, 4, 128, 3, tag="capped").name),
          "k1": ("wgrad_k1", _case("wgrad_k1", 1, 262400, 4, 4, 1, db=True, tag="capped").name),
          "f32": ("wgrad", _case("wgrad", 1, 131201, 1, 4, 2, tag="capped").name)}


def ariths_of(case):
    """the arithmetics whose kernels run this case (anything else must be refused: `refused_ariths`)"""
    if case.kind == "gelu":
        return ("f16x3",)
    if case.regime in F16_ONLY_REGIMES:
        return ("f16x3",)
    if case.kind == "wgrad":
        return ARITHS if case.k in WGRAD_RU else ("f32",)
    if case.kind == "wgrad_k1":
        return ARITHS
    return ARITHS if case.k <= SPLIT_KMAX else ("f32",)


def refused_ariths(case):
    """the split entry points that must answer IGN_E_UNSUP and touch nothing: more than 16 taps, or a weight gradient whose tap
    count has no split kernel"""
    if case.k > SPLIT_KMAX or (case.kind == "wgrad" and case.k not in WGRAD_RU):
        return SPLIT_ARITHS
    return ()


def runs():
    return [(c, a) for c in CASES for a in ariths_of(c)]


def find(kind, name):
    return next(c for c in CASES if c.kind == kind and c.name == name)


def dims(case):
    """-> (rows per sample of the output, reduction channels, output columns) of the NT kinds"""
    if case.kind in ("fwd",):
        return case.Tin - case.k + 1, case.Ci, case.Co
    return case.Tin, case.Co, case.Ci


def plan_of(arith, case):
    if case.kind in ("wgrad", "wgrad_k1"):
        return wgrad_plan(arith, case)
    rows, C, N = dims(case)
    epi = {"fwd": "bias", "dgrad": "mask", "dgrad_input": "plain", "gelu": "gelu"}[case.kind]
    return nt_plan(arith, case.B, rows, C, N, case.k, case.pro, epi, case.part and case.kind in ("fwd", "dgrad"))


# ----------------------------------------------------------------------------------------------------------------- the inputs
DRAWS = 8


def _gen(case, draw):
    return torch.Generator().manual_seed(zlib.crc32(f"{case.kind} {case.name} {draw}".encode()))


def _away_from_kink(y, a, b, margin=1e-3):
    pre = y * a + b
    return torch.where(pre.abs() < margin, y + 4 * margin / a, y)


def _magnitudes(shape, g):
    """sign * U(0.5, 2): no element far below the bound's scale (the two f16x3 regimes that waste ten bits of the bound)"""
    return (torch.rand(shape, generator=g) * 1.5 + 0.5) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def _pair(t, dim, g, negate):
    """odd index along `dim` = even index * (1 + 2^-9 r), r in (-1, 1)  |  = -even index"""
    even = t.index_select(dim, torch.arange(0, t.shape[dim] - t.shape[dim] % 2, 2))
    odd = -even if negate else (even.double() * (1 + 2.0 ** -9 * (torch.rand(even.shape, generator=g, dtype=torch.float64) * 2 - 1))).float()
    out = t.clone()
    out.index_copy_(dim, torch.arange(1, t.shape[dim], 2), odd)
    return out


@functools.lru_cache(maxsize=8)
def _draw_inputs(case, draw):
    """float32 CPU tensors of a case.  `a`, `b`: the two GEMM operands as the kernel stages them (`a` after the prologue, exactly:
    fmaxf(fmaf(pa, x, pb), 0) is one rounding of a sum float64 holds exactly); `bound_a`, `bound_b`: the f16x3 magnitude bounds."""
    g = _gen(case, draw)
    B, Tin, Ci, Co, k, regime = case.B, case.Tin, case.Ci, case.Co, case.k, case.regime
    Tout = Tin - k + 1
    d = {}
    rand = lambda *s: torch.randn(*s, generator=g)
    mags = regime in F16_ONLY_REGIMES
    if regime == "coarse":
        rand = lambda *s: torch.randint(-64, 65, s, generator=g).float() / 64
    if case.kind == "fwd":
        x = _magnitudes((B, Tin, Ci), g) if mags else rand(B, Tin, Ci)
        w = rand(Co, Ci, k) / (1 if regime == "coarse" else (Ci * k) ** 0.5)
        if regime == "pairs":
            x, w = _pair(x, 2, g, False), _pair(w, 1, g, True)
        if regime == "offset":
            x = x + 1000.0
            w = (w.double() - w.double().mean((1, 2), keepdim=True)).float()
        d.update(x=x, w=w, bias=rand(Co))
        if case.pro:
            d.update(pa=torch.rand(Ci, generator=g) + 0.5, pb=rand(Ci) * 0.3)
        op = "x"
    elif case.kind in ("dgrad", "dgrad_input", "gelu"):
        dy = _magnitudes((B, Tout, Co), g) if mags else rand(B, Tout, Co)
        w = rand(Co, Ci, k) / (Co * k) ** 0.5
        if regime == "pairs":
            dy, w = _pair(dy, 2, g, False), _pair(w, 0, g, True)
        if regime == "offset":
            dy = dy + 1000.0
            w = (w.double() - w.double().mean((0, 2), keepdim=True)).float()
        d.update(dy=dy, w=w)
        if case.kind == "dgrad":
            ea, eb = torch.rand(Ci, generator=g) + 0.5, rand(Ci) * 0.3
            d.update(ea=ea, eb=eb, emean=rand(Ci) * 0.2, einv=torch.rand(Ci, generator=g) + 0.5, y_in=_away_from_kink(rand(B, Tin, Ci), ea, eb))
        if case.kind == "gelu":
            d.update(u=rand(B, Tin, Ci) * 1.5)
        op = "dy"
    else:                                                                # wgrad, wgrad_k1: operands dy (rows x Co) and x (rows x Ci)
        x = _magnitudes((B, Tin, Ci), g) if mags else rand(B, Tin, Ci)
        dy = rand(B, Tout, Co)
        if regime == "pairs":                 # along a reduction index: the rows (k = 1), or the samples, which pairs every tap
            dim = 1 if case.kind == "wgrad_k1" else 0
            x, dy = _pair(x, dim, g, False), _pair(dy, dim, g, True)
        if regime == "offset":
            x = x + 1000.0
            dy = (dy.double() - dy.double().mean((0, 1), keepdim=True)).float()
        d.update(x=x, dy=dy)
        if case.pro:
            d.update(pa=torch.rand(Ci, generator=g) + 0.5, pb=rand(Ci) * 0.3)
        op = "x"
    if regime == "spike":
        d[op].view(-1)[d[op].numel() // 3] *= 1024.0
    a = d[op]
    if case.pro:
        a = torch.relu(a.double() * d["pa"].double() + d["pb"].double()).float()
    d["a"] = a
    d["b"] = d["w"] if "w" in d else d["dy"]                             # the other operand
    d["bound_a"] = float(a.abs().max()) * (1024.0 if regime == "loose" else 1.0)
    d["bound_b"] = float(d["b"].abs().max())
    return d


# -------------------------------------------------------------------------------------------------- the products and the models
def product(case, a, b):
    """the bilinear form of the case's kind on any dtype: (activation, weight) -> y, (gradient, weight) -> input gradient,
    (activation, gradient) -> dW (Co, Ci, k)"""
    if case.kind == "fwd":
        return F.conv1d(a.permute(0, 2, 1), b).permute(0, 2, 1)
    if case.kind in ("dgrad", "dgrad_input", "gelu"):
        return F.conv_transpose1d(a.permute(0, 2, 1), b).permute(0, 2, 1)
    Tout = case.Tin - case.k + 1
    return torch.stack([torch.einsum("bto,bti->oi", b, a[:, j:j + Tout]) for j in range(case.k)], dim=2)


def split_bf16(t, n=3):
    """x = x0 + x1 + x2, each the bf16 rounding of what is left (split3 of the kernels); float64 planes"""
    planes, r = [], t.float()
    for _ in range(n):
        p = r.bfloat16().float()
        planes.append(p.double())
        r = r - p
    return planes


def pow2_scale(bound):
    """ign_pow2_scale: 2^e with 2^13 <= bound * 2^e < 2^14"""
    if not (bound > 0 and bound < math.inf):
        return 1.0
    e = 14 - math.frexp(float(torch.tensor(bound, dtype=torch.float32)))[1]
    return math.ldexp(1.0, max(-60, min(60, e)))


def split_f16(t, bound):
    """two fp16 planes of the operand scaled by a power of two, scaled back (exactly) in float64"""
    s = pow2_scale(bound)
    v = t.float() * s
    h0 = v.half().float()
    h1 = (v - h0).half().float()
    return [h0.double() / s, h1.double() / s]


def operand_planes(d, arith):
    """-> (planes of a, planes of b, the (i, j) plane pairs the arithmetic multiplies)"""
    if arith == "bf16x6":
        return split_bf16(d["a"]), split_bf16(d["b"]), [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]
    if arith == "f16x3":
        return split_f16(d["a"], d["bound_a"]), split_f16(d["b"], d["bound_b"]), [(0, 0), (0, 1), (1, 0)]
    if arith == "bf16":
        return split_bf16(d["a"], 1), split_bf16(d["b"], 1), [(0, 0)]
    return [d["a"].double()], [d["b"].double()], [(0, 0)]


def model(case, arith, drop=(), d=None):
    """float64 sum of the plane products the arithmetic keeps (`drop`: pairs left out -- the planted defects)"""
    pa, pb, pairs = operand_planes(d if d is not None else inputs(case), arith)
    out = None
    for i in range(len(pa)):                                            # bilinear: one product per plane of a
        js = [j for (ii, j) in pairs if ii == i and (i, j) not in drop]
        if js:
            t = product(case, pa[i], sum(pb[j] for j in js))
            out = t if out is None else out + t
    return out


Bound = namedtuple("Bound", "exact cond e_model e_acc tol cap K")


def _draw_bound(case, arith, draw):
    d = _draw_inputs(case, draw)
    if arith == "bf16":                                                  # held to the product of the rounded operands
        a, b = d["a"].bfloat16().float(), d["b"].bfloat16().float()
    else:
        a, b = d["a"], d["b"]
    exact = product(case, a.double(), b.double())
    cond = product(case, a.double().abs(), b.double().abs())
    if case.kind == "fwd":
        cond = cond + d["bias"].double().abs()
    unit = U * cond.clamp_min(1e-300)
    e_model = 0.0 if arith in ("f32", "bf16") else float(((model(case, arith, d=d) - exact).abs() / unit).max())
    e_acc = float(((product(case, a, b).double() - exact).abs() / unit).max())
    K = plan_of(arith, case)["K"]
    return Bound(exact, cond, e_model, e_acc, e_model + max(TOL_FLOOR, TOL_FACTOR * e_acc), min(TOL_CAP, K + 8.0), K)


@functools.lru_cache(maxsize=None)
def _drawn(case):
    """The draw a case uses and its bounds under every arithmetic that runs it.  The tolerance of a draw is a property of the
    reference side alone (float64, its float32 evaluation, the float64 split emulation); the cap on it is a condition on the
    INPUTS, so a case takes the first of `DRAWS` seeds whose tolerance is under the cap for all its arithmetics.  Nothing the
    kernels compute enters the choice.  (No such draw: the last one stands and tests/test_conv_edges_host.py fails on the cap.)"""
    for draw in range(DRAWS):
        bounds = {a: _draw_bound(case, a, draw) for a in ariths_of(case)}
        if all(b.tol <= b.cap for b in bounds.values()):
            break
    return draw, bounds


def draw_of(case):
    return _drawn(case)[0]


def inputs(case):
    return _draw_inputs(case, draw_of(case))


def bound(case, arith):
    """exact float64 result (before bias / mask / GELU factor), cond, and the tolerance in units of u * cond"""
    return _drawn(case)[1][arith]


Ref = namedtuple("Ref", "ref cond extra tol")


def reference(case, arith):
    """-> name -> Ref: the float64 value each output must have and its element bound u * (tol * cond + extra)"""
    d, bd = inputs(case), bound(case, arith)
    zero = torch.zeros((), dtype=torch.float64)
    if case.kind == "fwd":
        return {"y": Ref(bd.exact + d["bias"].double(), bd.cond, zero, bd.tol)}
    if case.kind == "dgrad":
        mask = (torch.addcmul(d["eb"].double(), d["ea"].double(), d["y_in"].double()).float() > 0).double()
        return {"g_in": Ref(bd.exact * mask, bd.cond * mask, zero, bd.tol)}
    if case.kind == "dgrad_input":
        return {"gx": Ref(bd.exact, bd.cond, zero, bd.tol)}
    if case.kind == "gelu":
        # du = acc * gelu'(u).  gelu' = Phi(u) + u phi(u) in fp32 through erff / expf: |gelu'| <= 1.13 and its absolute error is at most
        # 8 u (two library calls of a few ulp each on values <= 1, one fma); the product adds half an ulp of the result
        u = d["u"].double()
        gp = 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
        return {"du": Ref(bd.exact * gp, bd.cond * gp.abs(), 8.0 * bd.exact.abs() + (bd.exact * gp).abs(), bd.tol)}
    out = {"dw": Ref(bd.exact, bd.cond, zero, bd.tol)}
    if case.db:
        # the bias gradient is a plain fp32 column sum of dy (no split): its own float32 evaluation sets its bound
        dy = d["dy"].double()
        ref, cond = dy.sum((0, 1)), dy.abs().sum((0, 1))
        e_acc = float(((d["dy"].sum((0, 1)).double() - ref).abs() / (U * cond)).max())
        out["db"] = Ref(ref, cond, zero, max(TOL_FLOOR, TOL_FACTOR * e_acc))
    return out


# ------------------------------------------------------------------------------------------------------------ planted defects
def defect_units(case, arith, what):
    """error of a float64 model with ONE planted defect, in units of u * cond: what the tolerance must be able to see"""
    d, bd = inputs(case), bound(case, arith)
    unit = U * bd.cond.clamp_min(1e-300)
    if what == "a1*b1 dropped":
        bad = model(case, "bf16x6", drop=((1, 1),))
    elif what == "h1*h0 dropped":
        bad = model(case, "f16x3", drop=((1, 0),))
    elif what == "padded channels read the neighbour":
        # channels C .. cp - 1 of the last chunk are zero on both sides; here both read on in memory instead: the activation into the
        # next row, the (co, tap, channel)-ordered weight into the next tap
        a, w = d["a"].double(), d["b"].double()
        wt = w.permute(0, 2, 1) if case.kind == "fwd" else w.flip(2).permute(1, 2, 0)        # (n, tap, c): the packed order
        ap = F.pad(a, (0, 0, case.k - 1, case.k - 1)) if case.kind != "fwd" else a
        n, k, c = wt.shape
        pad = kpad(c) - c
        assert pad > 0
        af = torch.cat([ap.reshape(ap.shape[0], -1), torch.zeros(ap.shape[0], pad, dtype=a.dtype)], 1)
        wf = torch.cat([wt.reshape(n, -1), torch.zeros(n, pad, dtype=a.dtype)], 1)
        R = ap.shape[1] - k + 1
        cols = torch.stack([af[:, (t + j) * c:(t + j) * c + c + pad] for t in range(R) for j in range(k)], 1).reshape(ap.shape[0], R, -1)
        wcols = torch.stack([wf[:, j * c:j * c + c + pad] for j in range(k)], 1).reshape(n, -1)
        bad = cols @ wcols.t()
    elif what == "one tap shifted by a row":
        a, w = d["a"].double(), d["b"].double()
        j0 = case.k // 2
        w1 = torch.zeros_like(w)
        w1[:, :, j0] = w[:, :, j0]
        bad = bd.exact - product(case, a, w1) + product(case, torch.roll(a, 1, dims=1), w1)
    elif what == "empty split returns stale data":
        p = wgrad_plan(arith, case)
        assert p["empty"] > 0
        # the reducer adds every split: an empty one that kept the first split's partial adds it a second time.  A probe of what the
        # tolerance sees, not the partial a kernel would leave: the multi-tap kernel's units never straddle a sample, so its first
        # split is not exactly the first per * ru rows of the flattened (sample, row) index that are taken here
        first = p["per"] * (p.get("ru", WGRAD_K1_UNIT)) if "per" in p else p["rows_per"]
        a, b = d["a"].double(), d["b"].double()
        flat_rows = torch.zeros(case.B * (case.Tin - case.k + 1), dtype=torch.bool)
        flat_rows[:min(first, flat_rows.numel())] = True
        keep = flat_rows.view(case.B, -1, 1).double()
        bad = bd.exact + product(case, a, b * keep)
    else:
        raise KeyError(what)
    return float(((bad - bd.exact).abs() / unit).max())
