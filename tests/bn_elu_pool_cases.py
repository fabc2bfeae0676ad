"""ops.bn_elu_pool -- BatchNorm2d (batch statistics) + ELU + AvgPool of the EEG-CNN blocks as one op over seven kernels of
csrc/ign_eegcnn_fused.hip -- at every edge of its launch arithmetic and in the value regimes where it can go wrong: the launch
arithmetic restated in Python (`plan_*`), the case table built from its branch points, float64 references written out in numpy, fp32
restatements in kernel order with seeded defects, and the tolerances.  numpy only.

Tolerance rule (the one of tests/glue_edge_cases.py).  u = 2^-24.  A sum is held to  d u sum|terms| + the elementwise roundings of
its terms (+ 1 ulp where the result is an fp32 value; the sums here leave the kernels as doubles), d the per-thread serial fp32 chain:
ceil(T / 256) in chan_stats_kernel, ceil(Tp P / 256) in bn_elu_pool_bwd_sums_kernel, P - 1 in affine_elu_pool_kernel, never above
D_CAP = 96.  The double stages (rows of a slice, the block reduction, the slices) add nothing.  The outputs of the two fold kernels
(scale, shift, mean, r, the running statistics; ka, kb, kc, dgamma, dbeta, dalpha) take the interval of the sums through the float64
formulas, evaluated at the interval ends, plus 2 ulp of their largest term -- through the C ABI the sums are an input, the interval is
empty and 2 ulp is all they get.  dalpha gets the relative bound of its channel's S2 (and of r^3) plus those 2 ulp, and no floor.
out is held per element to  K_OUT u (|scale v| + |shift|)  for the argument of ELU (two roundings of coefficients and one fma, with
the 4x of headroom the host test asks for: 8), C_EXPM1 ulp for expm1f, the P - 1 additions and one ulp for the division; dv to
K_DV u (|ka dz| + |kc v| + |kb|) (three coefficients, two fmas: 12); both plus what the coefficient intervals do to the element.  ELU'
is __expf: exp2 of the fp32 product z log2(e), relative error (|z| log2 e + C_EXPF) 2^-23, and an error dz of its argument changes it
by expm1(dz) relative -- which also covers an element whose z changes sign within dz, ELU' being continuous at 0.  Rounding the saved
mean to fp32 for the backward sums enters S2 as u |m| sum|dz|.  In the `exact` regime (v in -3..3, P a power of two, integer dout and
mean, z > 0 everywhere) no fp32 operation rounds: ign_chan_stats, ign_bn_elu_pool_bwd_sums, ign_affine_elu_pool_fwd and
ign_bn_elu_pool_bwd_apply must equal float64.

C_EXPM1 and C_EXPF are not stated by the documentation at hand; they were measured for the two intrinsics alone (ELU at P = 1, scale
1, shift 0 is expm1f itself; the apply kernel at P = 1, ka = 1, kb = kc = 0, dout = 1 is __expf itself) and doubled:
profiles/bn_elu_pool_edges.json, "intrinsics".  Nothing else here is read from a kernel's output."""
import functools
import zlib

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
ULP = 2.0 ** -23
TINY = 2.0 ** -126
D_CAP = 96
IGN_E_ARG = -1001
LOG2E = 1.4426950408889634

# constants of csrc/ign_eegcnn_fused.hip (tests/test_bn_elu_pool_host.py parses the source and compares)
THREADS, SLICE_CAP, FOLD_BLOCK, FIN_BLOCK = 256, 32, 64, 128
BN_C_MAX, BN_BC_MAX, BN_T_MAX = 65535, 2 ** 31 - 1, 65535 * 256

C_EXPM1 = 1.8          # ulp of expm1f: 2 x the measured 0.89 (profiles/bn_elu_pool_edges.json: intrinsics.expm1f)
C_EXPF = 1.6           # ulp of the hardware exp2 inside __expf: 2 x the measured 0.78 (intrinsics.expf_vs_exp2_of_fp32_product)
K_OUT, K_DV = 8, 12
K_DZ = 3               # ELU' * dout * (1/P): two products and the rounded reciprocal (resp. one product and one division)

EPS32 = float(f32(1e-5))          # nn.BatchNorm2d's defaults as the ABI receives them (floats)
MOM32 = float(f32(0.1))
CONST_X, CONST_SHORTFALL = 63.0 / 64.0 + 2.0 ** -13, 2.0 ** -26       # fl32(x^2) = x^2 - 2^-26
MIN_DALPHA_OVER_DGAMMA = 1e-2


def cdiv(a, b):
    return -(-a // b)


# ============================================================================================================ launch arithmetic
def stat_slices(B):
    return max(1, min(B, SLICE_CAP))


def bn_refuses(B, C, T, P):
    return B <= 0 or C <= 0 or T <= 0 or P <= 0 or P > T or C > BN_C_MAX or B * C > BN_BC_MAX or T > BN_T_MAX


def _chain_classes(tag, n):
    """per-thread chain over n elements of a row with 256 threads"""
    chain = cdiv(n, THREADS)
    cls = {f"{tag}:chain1" if chain == 1 else f"{tag}:chain2" if chain == 2 else f"{tag}:chain>2"}
    if n % THREADS:
        cls.add(f"{tag}:ragged_chain")            # the last pass is taken by some threads only
    else:
        cls.add(f"{tag}:full_chain")
    if n < 64:
        cls.add(f"{tag}:three_idle_waves")        # block_sum2 sums three waves of zeros
    elif n < THREADS - 64 + 1:
        cls.add(f"{tag}:idle_waves")
    return chain, cls


def _slice_classes(tag, B):
    nsl = stat_slices(B)
    rows = {len(range(s, B, nsl)) for s in range(nsl)}
    cls = {f"{tag}:B1" if B == 1 else f"{tag}:B<=32" if B <= SLICE_CAP else f"{tag}:B>32"}
    if B == SLICE_CAP:
        cls.add(f"{tag}:B=32")
    if B > SLICE_CAP:
        cls.add(f"{tag}:uneven_slices" if len(rows) > 1 else f"{tag}:even_slices")
    return nsl, rows, cls


def plan_fold(C):
    blocks, fin_blocks = cdiv(C, FOLD_BLOCK), cdiv(2 * C, FIN_BLOCK)
    cls = {"fold:C1" if C == 1 else "fold:one_block" if blocks == 1 else "fold:many_blocks",
           "fold:full_block" if C % FOLD_BLOCK == 0 else "fold:ragged_block",
           "fin:full_block" if (2 * C) % FIN_BLOCK == 0 else "fin:ragged_block",
           "fin:one_block" if fin_blocks == 1 else "fin:two_blocks" if fin_blocks == 2 else "fin:three_blocks",
           "rowmap:C1" if C == 1 else "rowmap:pow2" if C & (C - 1) == 0 else "rowmap:not_pow2", "fold:dalpha", "fold:running"}
    return dict(route=f"fold {blocks} x {FOLD_BLOCK}, finalize {fin_blocks} x {FIN_BLOCK}", blocks=blocks, fin_blocks=fin_blocks,
                classes=cls)


def plan_stats(B, C, T):
    nsl, rows, c1 = _slice_classes("stats", B)
    chain, c2 = _chain_classes("stats", T)
    idle = max(0, THREADS // 64 - cdiv(T, 64))
    return dict(route=f"chan_stats_kernel grid ({C},{nsl}), rows/slice {sorted(rows)}, chain {chain}, {idle} idle waves", slices=nsl,
                rows_per_slice=rows, chain=chain, idle_waves=idle, classes=c1 | c2)


def plan_pool(T, P):
    Tp, ny = T // P, cdiv(T // P, THREADS)
    rem = T - Tp * P
    cls = {"pool:P1" if P == 1 else "pool:P=T" if P == T else "pool:P>1",
           "pool:rem0" if rem == 0 else "pool:rem=P-1" if rem == P - 1 else "pool:rem_mid",
           "pool:ny1" if ny == 1 else "pool:ny2" if ny == 2 else "pool:ny>2",
           "pool:full_block" if Tp % THREADS == 0 else "pool:ragged_block"}
    if Tp == 1:
        cls.add("pool:Tp1")
    if Tp in (THREADS, THREADS + 1):
        cls.add(f"pool:Tp={Tp}")
    return dict(route=f"affine_elu_pool_kernel grid.y {ny}, Tp {Tp}, remainder {rem}", Tp=Tp, rem=rem, ny=ny, chain=max(P - 1, 0),
                classes=cls)


def plan_bwd(B, C, T, P):
    Tp = T // P
    rem = T - Tp * P
    nsl, rows, c1 = _slice_classes("bwd", B)
    chain, c2 = _chain_classes("bwd", Tp * P)
    ny = cdiv(T, THREADS)
    cls = c1 | c2 | {"bwd:remainder" if rem else "bwd:no_remainder", "apply:ny1" if ny == 1 else "apply:ny2" if ny == 2 else "apply:ny>2",
                     "apply:full_block" if T % THREADS == 0 else "apply:ragged_block"}
    if rem and rem == P - 1:
        cls.add("bwd:remainder=P-1")
    if P > 1:
        cls.add("bwd:shared_dout")               # tt / P: P elements read one dout
    return dict(route=f"bn_elu_pool_bwd_sums_kernel grid ({C},{nsl}), chain {chain}; bn_elu_pool_bwd_apply_kernel grid.y {ny}, "
                      f"remainder {rem}", slices=nsl, rows_per_slice=rows, chain=chain, ny=ny, rem=rem, Tp=Tp, classes=cls)


def plan(c):
    ps = [plan_stats(c.B, c.C, c.T), plan_pool(c.T, c.P), plan_bwd(c.B, c.C, c.T, c.P), plan_fold(c.C)]
    return dict(route="; ".join(p["route"] for p in ps), classes=set().union(*[p["classes"] for p in ps]))


def all_classes():
    """every class a plan can return, by enumerating the axes around every constant"""
    out = set()
    for B in (1, 2, 31, 32, 33, 64, 65):
        for T in (1, 2, 63, 64, 65, 192, 193, 255, 256, 257, 512, 513, 1285):
            out |= plan_stats(B, 1, T)["classes"]
            for P in (1, 2, 5, T):
                if P <= T:
                    out |= plan_pool(T, P)["classes"] | plan_bwd(B, 1, T, P)["classes"]
    for C in (1, 2, 3, 63, 64, 65, 128, 129):
        out |= plan_fold(C)["classes"]
    return out


# ============================================================================================================ the table
OP_REGIMES = ("gauss", "offset16", "offset256", "epsdom_small", "epsdom_eps", "constant")
DIRECT_REGIMES = ("exact", "zero_crossing", "saturated")


class Case:
    def __init__(self, regime, B, C, T, P, affine=True, bn_affine=True):
        self.regime, self.B, self.C, self.T, self.P, self.affine, self.bn_affine = regime, B, C, T, P, affine, bn_affine
        self.name = f"B{B}-C{C}-T{T}-P{P}" + ("" if affine else "-noalpha") + ("" if bn_affine else "-bnplain")
        self.id = f"{self.name}-{regime}"
        self.direct = regime in DIRECT_REGIMES
        self.exact = regime == "exact"

    def __repr__(self):
        return self.id


# (B, C, T, P): the axes B 1, 2, 31, 32, 33, 64, 65 / C 1, 3, 63, 64, 65, 129 / T 2, 63, 64, 65, 255, 256, 257, 513, 1285 /
# P 1, 2, 5, T, paired where they meet in one plan; the large B sit on small C T and the reverse
SHAPES = [
    (1, 1, 2, 1), (1, 3, 2, 2), (65, 3, 2, 2), (2, 3, 63, 2), (2, 3, 63, 63), (2, 1, 64, 1), (31, 3, 64, 5), (31, 3, 65, 5),
    (32, 3, 255, 2), (33, 3, 256, 1), (33, 5, 257, 1), (65, 1, 257, 2), (3, 3, 257, 257), (64, 3, 513, 2), (1, 3, 513, 1),
    (2, 3, 1285, 5), (2, 3, 1285, 2), (31, 1, 513, 5), (2, 63, 64, 2), (2, 64, 65, 2), (2, 65, 64, 5), (1, 129, 255, 5),
    (2, 129, 63, 1), (33, 63, 65, 5), (3, 64, 256, 2),
]
# offset: |mean| / sigma of 16 and of 256 (tests/test_bn_elu_pool_host.py shows the restatement keeps 4x headroom at 256: the bound
# grows with the offset as the error does, so the ratio was not lowered)
OFFSET_SHAPES = [(2, 3, 63, 2), (33, 3, 256, 1), (2, 3, 1285, 5), (2, 65, 64, 5)]
EPSDOM_SHAPES = [(2, 3, 63, 2), (33, 5, 257, 1), (2, 64, 65, 2), (31, 3, 65, 5)]
CONSTANT_SHAPES = [(2, 3, 63, 2), (33, 3, 256, 1), (31, 3, 65, 5)]          # T <= 256: q / n - m^2 = -2^-26 exactly in channel 1
DIRECT_SHAPES = [(2, 3, 63, 2), (33, 5, 257, 1), (2, 3, 1285, 5), (65, 3, 2, 2)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for i, s in enumerate(SHAPES):
        out.append(Case("gauss", *s, affine=i % 3 != 2))
        if s[3] & (s[3] - 1) == 0:
            out.append(Case("exact", *s))
    out += [Case(r, *s) for s in OFFSET_SHAPES for r in ("offset16", "offset256")]
    out += [Case(r, *s) for s in EPSDOM_SHAPES for r in ("epsdom_small", "epsdom_eps")]
    out += [Case("constant", *s) for s in CONSTANT_SHAPES]
    out += [Case(r, *s) for s in DIRECT_SHAPES for r in ("zero_crossing", "saturated")]
    assert len({c.id for c in out}) == len(out)
    return out


def op_cases():
    return [c for c in cases() if not c.direct]


REFUSALS = [dict(B=2, C=3, T=10, P=11, why="P > T"), dict(B=2, C=3, T=10, P=0, why="P = 0"), dict(B=2, C=3, T=10, P=-1, why="P < 0")]

# ops.bn_elu_pool host branches: (name, BatchNorm2d keywords, training)
HOST_BRANCHES = [("cumulative", dict(momentum=None), True), ("no_tracking_train", dict(track_running_stats=False), True),
                 ("no_tracking_eval", dict(track_running_stats=False), False), ("no_affine", dict(affine=False), True),
                 ("no_affine_eval", dict(affine=False), False)]
HOST_SHAPE = (5, 3, 70, 4)                  # remainder 2

# the EEG-CNN row: a MODEL_CASES-sized shape on the "fold" route, input at 1e-3 of unit variance (a recording kept in volts)
MODEL_ROW = dict(shape=(6, 9, 200, 31, 25, 4, 2, 2, 4), input_scale=1e-3, fp32_factor=4.0)


# ============================================================================================================ inputs
def _rng(c):
    return np.random.default_rng(zlib.crc32(c.id.encode()))


def _ints(g, lo, hi, *shape):
    return g.integers(lo, hi + 1, size=shape).astype(f32)


def _pow2(g, lo, hi, n):
    return (f32(2.0) ** g.integers(lo, hi + 1, size=n).astype(f32)) * np.where(g.random(n) > 0.5, 1, -1).astype(f32)


@functools.lru_cache(maxsize=8)
def inputs(c):
    g = _rng(c)
    B, C, T, P = c.B, c.C, c.T, c.P
    Tp = T // P
    sign = np.where(g.random(C) > 0.3, 1.0, -1.0)
    sign[0] = 1.0
    sign[-1] = -1.0 if C > 1 else 1.0
    d = dict(alpha=((g.random(C) + 0.5) * sign).astype(f32), cshift=g.standard_normal(C).astype(f32),
             gamma=g.uniform(0.5, 1.5, C).astype(f32), beta=g.uniform(-0.5, 0.5, C).astype(f32), eps=EPS32, momentum=MOM32,
             run_mean=g.standard_normal(C).astype(f32), run_var=g.uniform(0.5, 2.0, C).astype(f32),
             dout=g.standard_normal((B, C, Tp)).astype(f32))
    z = g.standard_normal((B, C, T))
    r = c.regime
    if r == "gauss":
        v = z * 1.7 + 0.3
    elif r.startswith("offset"):
        v = z + float(r[6:]) * sign[None, :, None]
    elif r == "epsdom_small":
        v = 1e-2 * z
    elif r == "epsdom_eps":
        v, d["eps"] = z, 0.5
    elif r == "constant":
        v = z
        v[:, 0, :] = 0.75
        if C > 1:
            v[:, 1, :] = CONST_X                      # fl32(x^2) = x^2 - 2^-26: the fp32 sum of squares falls short of n m^2
            d["alpha"][1] = 1.0
        d["eps"] = CONST_SHORTFALL / 4                # below the shortfall: without the clamp 1 / sqrt of a negative number
    elif r == "exact":
        v = _ints(g, -3, 3, B, C, T)
        d["dout"] = _ints(g, -4, 4, B, C, Tp)
        d["scale"] = _pow2(g, 0, 1, C)
        d["shift"] = (3 * np.abs(d["scale"]) + _ints(g, 1, 4, C)).astype(f32)
        d["mean"] = _ints(g, -2, 2, C)
        d["ka"], d["kc"], d["kb"] = _pow2(g, -1, 1, C), _pow2(g, -3, -2, C), _ints(g, -3, 3, C)
    elif r == "zero_crossing":
        v = z
        v[g.random((B, C, T)) < 0.25] = 0.5
        d["scale"] = _pow2(g, 1, 1, C)
        d["shift"] = (-0.5 * d["scale"]).astype(f32)
    elif r == "saturated":
        v = z
        d["scale"] = (g.uniform(0.5, 1.5, C) * sign).astype(f32)
        vmax = np.abs(v.astype(f32)).max(axis=(0, 2))
        deep = g.uniform(0, 60, C)
        deep[0] = 75.0                                # channel 0: below -88 everywhere, __expf underflows
        d["shift"] = (-20.5 - np.abs(d["scale"]) * vmax * 1.001 - deep).astype(f32)
    else:
        raise ValueError(r)
    d["v"] = np.ascontiguousarray(v, dtype=f32)
    if r in ("zero_crossing", "saturated"):
        d["mean"] = (0.1 * g.standard_normal(C)).astype(f32)
        d["ka"], d["kb"], d["kc"] = (g.standard_normal(C).astype(f32) for _ in range(3))
    if not c.affine:
        d["alpha"] = d["cshift"] = None
    if not c.bn_affine:           # BatchNorm2d(affine=False): the identity affine map
        d["gamma"], d["beta"] = np.ones(C, f32), np.zeros(C, f32)
    return d


# ============================================================================================================ float64 formulas
def moments64(v):
    """-> s, q, sum|v| per channel"""
    x = v.astype(f64)
    return x.sum(axis=(0, 2)), (x * x).sum(axis=(0, 2)), np.abs(x).sum(axis=(0, 2))


def fold_fwd64(s, q, n, d, momentum=None, defect=None, run=None, centred=None):
    """y = alpha v + c;  mean, var (biased, clamped at 0) of v;  r = 1 / sqrt(alpha^2 var + eps);  scale = gamma alpha r;
    shift = beta - scale mean  (`centred`: the same about a two-pass variance, for the reference);  running_mean <- (1 - mom) running_mean + mom (alpha mean + c);
    running_var <- (1 - mom) running_var + mom alpha^2 var n / (n - 1)   (n = 1: the biased one)"""
    C = len(s)
    a = d["alpha"].astype(f64) if d["alpha"] is not None else np.ones(C)
    cs = d["cshift"].astype(f64) if d["cshift"] is not None else np.zeros(C)
    g, b = d["gamma"].astype(f64), d["beta"].astype(f64)
    m = s / n
    if centred is None:
        var = np.maximum(q / n - m * m, 0.0)
    else:             # (s0, q0, var0), var0 the two-pass variance at (s0, q0): no cancellation under a DC offset
        s0, q0, var0 = centred
        var = np.maximum(var0 + (q - q0) / n - (m - s0 / n) * (m + s0 / n), 0.0)
    r = 1.0 / np.sqrt(a * a * var + d["eps"])
    sc = g * a * r
    out = dict(scale=sc, shift=b - sc * m, mean=m, r=r, var=var)
    big = dict(scale=np.abs(sc), shift=np.abs(b) + np.abs(sc * m), mean=np.abs(m), r=r)
    mom = d["momentum"] if momentum is None else momentum
    rm, rv = run if run is not None else (d["run_mean"].astype(f64), d["run_var"].astype(f64))
    unb = 1.0 if (n <= 1 or defect == "biased_running_var") else n / (n - 1.0)
    out["run_mean"] = (1 - mom) * rm + mom * (a * m + cs)
    out["run_var"] = (1 - mom) * rv + mom * a * a * var * unb
    big["run_mean"] = np.abs((1 - mom) * rm) + np.abs(mom * a * m) + np.abs(mom * cs)
    big["run_var"] = np.abs(out["run_var"])
    return out, big


def elu_grad_terms64(v, dout, scale, shift, P):
    """-> z, dz, |dout| / P over (B, C, T) in float64 (the last two 0 on the pooling remainder)"""
    B, C, T = v.shape
    Tp = T // P
    z = scale.astype(f64)[None, :, None] * v.astype(f64) + shift.astype(f64)[None, :, None]
    g = np.where(z > 0, 1.0, np.exp(np.minimum(z, 0.0)))
    w = np.zeros((B, C, T))
    w[:, :, :Tp * P] = np.repeat(dout.astype(f64), P, axis=2) / P
    return z, g * w, np.abs(w)


def pool64(z, P):
    B, C, T = z.shape
    Tp = T // P
    e = np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))
    return e[:, :, :Tp * P].reshape(B, C, Tp, P)


def fold_bwd64(S1, S2, m, r, d, n, defect=None):
    """ka = gamma alpha r;  kc = -ka alpha^2 r^2 S2 / n;  kb = -ka S1 / n - kc mean;  dgamma = alpha r S2;  dbeta = S1;
    dalpha = gamma r^3 eps S2"""
    C = len(S1)
    a = d["alpha"].astype(f64) if d["alpha"] is not None else np.ones(C)
    g = d["gamma"].astype(f64)
    k0 = g * a * r
    kc = -k0 * a * a * r * r * S2 / n
    mk = m.astype(f32).astype(f64) if defect == "mean_rounding_in_kb" else m
    out = dict(ka=k0, kc=kc, kb=-k0 * S1 / n - kc * mk, dgamma=a * r * S2, dbeta=S1)
    big = dict(ka=np.abs(k0), kc=np.abs(kc), kb=np.abs(k0 * S1 / n) + np.abs(kc * m), dgamma=np.abs(out["dgamma"]), dbeta=np.abs(S1))
    if d["alpha"] is not None:
        da = g * r * r * r * d["eps"] * S2
        if defect == "dalpha_sign":
            da = -da
        if defect == "dalpha_no_eps":
            da = g * r * S2
        out["dalpha"], big["dalpha"] = da, np.abs(g * r * r * r * d["eps"] * S2)
    return out, big


# ============================================================================================================ references
class Ref:
    """ref (float64), tol (float64, same shape; 0 = must be equal)"""

    def __init__(self, ref, tol):
        self.ref = np.asarray(ref, f64)
        self.tol = np.broadcast_to(np.asarray(tol, f64), self.ref.shape).copy()


def _corners(f, centre, halves):
    """max over the corners of the box centre +- halves of |f(corner) - f(centre)|, per key"""
    mid = f(*centre)
    half = {k: np.zeros_like(np.asarray(x, f64)) for k, x in mid.items()}
    for bits in range(1 << len(centre)):
        pt = [x + (1 if bits >> i & 1 else -1) * h for i, (x, h) in enumerate(zip(centre, halves))]
        for k, x in f(*pt).items():
            half[k] = np.maximum(half[k], np.abs(x - mid[k]))
    return mid, half


def stats_ref(c, d):
    s, q, sa = moments64(d["v"])
    if c.exact:
        return dict(s=Ref(s, 0.0), q=Ref(q, 0.0))
    dd = min(cdiv(c.T, THREADS), D_CAP)
    return dict(s=Ref(s, dd * U * sa + TINY), q=Ref(q, (dd + 1) * U * q + TINY))


def _dz_err(z, dz, hz, w):
    """what ELU' and the two products can be off by, per element: hz = bound on the error of z, w = |dout| / P (an ELU' below the
    smallest normal number is flushed to zero: 2^-126 absolute)"""
    rel = np.expm1(np.minimum(hz, 1.0)) + np.where(z > 0, 0.0, (np.abs(z) * LOG2E + C_EXPF) * ULP) + K_DZ * U
    return np.abs(dz) * rel + 2 * TINY * w + TINY


def fwd_ref(c, v, scale, shift, hz=0.0, exact=False):
    """out and its bound from coefficients taken as given (hz: what their own error does to z, per element)"""
    z = scale.astype(f64)[None, :, None] * v.astype(f64) + shift.astype(f64)[None, :, None]
    e = pool64(z, c.P)
    out = e.mean(axis=3)
    if exact:
        return Ref(out, 0.0)
    P, Tp = c.P, c.T // c.P
    ez = K_OUT * U * (np.abs(scale.astype(f64))[None, :, None] * np.abs(v.astype(f64)) + np.abs(shift.astype(f64))[None, :, None]) + hz
    ez = ez[:, :, :Tp * P].reshape(e.shape)
    ee = ez + C_EXPM1 * ULP * np.abs(e) + TINY
    return Ref(out, ee.mean(axis=3) + min(P - 1, D_CAP) * U * np.abs(e).mean(axis=3) + ULP * np.abs(out) + TINY)


def bwd_sums_ref(c, v, dout, scale, shift, mean, hz=0.0, hm=0.0, exact=False):
    """S1, S2 about `mean` (float64 per channel); hm: bound on the error of the mean the kernel is given"""
    z, dz, w = elu_grad_terms64(v, dout, scale, shift, c.P)
    vc = v.astype(f64) - mean[None, :, None]
    S1, S2 = dz.sum(axis=(0, 2)), (dz * vc).sum(axis=(0, 2))
    if exact:
        return dict(S1=Ref(S1, 0.0), S2=Ref(S2, 0.0)), z, dz
    sc64, sh64 = np.abs(scale.astype(f64))[None, :, None], np.abs(shift.astype(f64))[None, :, None]
    ez = U * (sc64 * np.abs(v.astype(f64)) + sh64) + hz                     # one fma on given coefficients
    edz = _dz_err(z, dz, ez, w)
    edz[:, :, (c.T // c.P) * c.P:] = 0.0
    dd = min(cdiv((c.T // c.P) * c.P, THREADS), D_CAP)
    t1 = edz.sum(axis=(0, 2)) + dd * U * np.abs(dz).sum(axis=(0, 2)) + TINY
    t2 = (edz * np.abs(vc)).sum(axis=(0, 2)) + (dd + 1) * U * np.abs(dz * vc).sum(axis=(0, 2)) + hm * np.abs(dz).sum(axis=(0, 2)) + TINY
    return dict(S1=Ref(S1, t1), S2=Ref(S2, t2)), z, dz


def apply_ref(c, v, dout, scale, shift, ka, kb, kc, hz=0.0, hk=(0.0, 0.0, 0.0), exact=False):
    z, dz, w = elu_grad_terms64(v, dout, scale, shift, c.P)
    col = lambda x: np.asarray(x, f64)[None, :, None]
    x = v.astype(f64)
    dv = col(ka) * dz + col(kc) * x + col(kb)
    if exact:
        return Ref(dv, 0.0)
    ez = K_OUT * U * (np.abs(col(scale)) * np.abs(x) + np.abs(col(shift))) + hz
    edz = _dz_err(z, dz, ez, w)
    edz[:, :, (c.T // c.P) * c.P:] = 0.0
    hka, hkb, hkc = (col(h) if np.ndim(h) else h for h in hk)
    tol = np.abs(col(ka)) * edz + hka * np.abs(dz) + hkc * np.abs(x) + hkb \
        + K_DV * U * (np.abs(col(ka) * dz) + np.abs(col(kc) * x) + np.abs(col(kb))) + TINY
    return Ref(dv, tol)


def _two_ulp(mid, big, keys):
    return {k: Ref(mid[k], 2 * ULP * big[k] + TINY) for k in keys if k in mid}


FOLD_FWD_OUT = ("scale", "shift", "mean", "r", "run_mean", "run_var")
FOLD_BWD_OUT = ("ka", "kb", "kc", "dgamma", "dbeta", "dalpha")


@functools.lru_cache(maxsize=4)
def direct(c):
    """The six entry points one by one, each on inputs it is GIVEN (what the stage before it would hand on, in kernel order, or the
    regime's own coefficients), each against float64 of those inputs.  -> (inputs of the later stages, entry -> output -> Ref)"""
    d = inputs(c)
    n = c.B * c.T
    give, refs = {}, {}
    refs["ign_chan_stats"] = stats_ref(c, d)
    give["sums"] = restate_stats(d["v"])                                    # (C, 2) doubles
    mid, big = fold_fwd64(give["sums"][:, 0], give["sums"][:, 1], n, d)
    refs["ign_bn_fold_fwd"] = _two_ulp(mid, big, FOLD_FWD_OUT)
    for k in ("mean", "r"):                                                 # doubles: no fp32 rounding
        refs["ign_bn_fold_fwd"][k] = Ref(mid[k], 8 * 2.0 ** -53 * big[k])
    give["scale"] = d["scale"] if "scale" in d else mid["scale"].astype(f32)
    give["shift"] = d["shift"] if "shift" in d else mid["shift"].astype(f32)
    give["mean"] = d["mean"] if "mean" in d else mid["mean"].astype(f32)
    give["fold"] = np.stack([mid["mean"], mid["r"]], axis=1)
    refs["ign_affine_elu_pool_fwd"] = dict(out=fwd_ref(c, d["v"], give["scale"], give["shift"], exact=c.exact))
    rs, _, _ = bwd_sums_ref(c, d["v"], d["dout"], give["scale"], give["shift"], give["mean"].astype(f64), exact=c.exact)
    refs["ign_bn_elu_pool_bwd_sums"] = rs
    S1, S2 = restate_bwd_sums(d["v"], d["dout"], give["scale"], give["shift"], give["mean"], c.P)
    give["bsums"] = np.stack([S1, S2], axis=1)
    bmid, bbig = fold_bwd64(S1, S2, mid["mean"], mid["r"], d, n)
    refs["ign_bn_fold_bwd"] = _two_ulp(bmid, bbig, FOLD_BWD_OUT)
    for k in ("ka", "kb", "kc"):
        give[k] = d[k] if k in d else bmid[k].astype(f32)
    refs["ign_bn_elu_pool_bwd_apply"] = dict(dv=apply_ref(c, d["v"], d["dout"], give["scale"], give["shift"], give["ka"], give["kb"],
                                                          give["kc"], exact=c.exact))
    return give, refs


@functools.lru_cache(maxsize=4)
def reference_op(c, momentum=None, calls=1):
    """ops.bn_elu_pool in training mode from the raw inputs, in float64, with the bound of every output: out, dv, dgamma, dbeta,
    dalpha, running statistics (after `calls` calls on the same batch; momentum=None: the cumulative average 1 / k), and the
    intermediate sums and coefficients.  dc is exactly 0 (c cancels in the normalisation)."""
    d = inputs(c)
    v, n, C = d["v"], c.B * c.T, c.C
    s, q, sa = moments64(v)
    d1 = min(cdiv(c.T, THREADS), D_CAP)
    ts, tq = d1 * U * sa, (d1 + 1) * U * q
    cen = (s, q, ((v.astype(f64) - (s / n)[None, :, None]) ** 2).sum(axis=(0, 2)) / n)

    def fwd(s_, q_):
        out, _ = fold_fwd64(s_, q_, n, d, centred=cen)
        return {k: out[k] for k in ("scale", "shift", "mean", "r")}
    mid, half = _corners(fwd, (s, q), (ts, tq))
    _, big = fold_fwd64(s, q, n, d, centred=cen)
    R = {k: Ref(mid[k], half[k] + 2 * ULP * big[k] + TINY) for k in mid}
    # running statistics: call k uses momentum (or 1 / k); every call's rounding is 2 ulp of its largest term
    run = (d["run_mean"].astype(f64), d["run_var"].astype(f64))
    lo = hi = run
    trm = trv = 0.0
    for k in range(1, calls + 1):
        mom = 1.0 / k if momentum == "cumulative" else d["momentum"]
        o, b = fold_fwd64(s, q, n, d, momentum=mom, run=run, centred=cen)

        def runf(s_, q_, mom=mom, run=run):
            oo, _ = fold_fwd64(s_, q_, n, d, momentum=mom, run=run, centred=cen)
            return dict(run_mean=oo["run_mean"], run_var=oo["run_var"])
        _, h = _corners(runf, (s, q), (ts, tq))
        trm = (1 - mom) * trm + h["run_mean"] + 2 * ULP * b["run_mean"]
        trv = (1 - mom) * trv + h["run_var"] + 2 * ULP * b["run_var"]
        run = (o["run_mean"], o["run_var"])
    R["run_mean"], R["run_var"] = Ref(run[0], trm + TINY), Ref(run[1], trv + TINY)
    # forward: z = scale (v - mean) + beta; the coefficient intervals move it by at most hz
    x = v.astype(f64)
    col = lambda a: np.asarray(a, f64)[None, :, None]
    hsc, hm = half["scale"] + 2 * ULP * big["scale"], half["mean"]
    hz = col(hsc) * np.abs(x - col(mid["mean"])) + col(np.abs(mid["scale"]) + hsc) * col(hm)
    R["out"] = fwd_ref(c, v, mid["scale"], mid["shift"], hz=hz)
    # backward sums about the float64 mean; the kernel is given the mean rounded to fp32
    rs, z, dz = bwd_sums_ref(c, v, d["dout"], mid["scale"], mid["shift"], mid["mean"],
                             hz=hz + (K_OUT - 1) * U * (col(np.abs(mid["scale"])) * np.abs(x) + col(np.abs(mid["shift"]))),
                             hm=hm + U * np.abs(mid["mean"]))
    R.update(rs)
    S1, S2, t1, t2 = rs["S1"].ref, rs["S2"].ref, rs["S1"].tol, rs["S2"].tol
    hr = half["r"]

    def bwd(S1_, S2_, m_, r_):
        out, _ = fold_bwd64(S1_, S2_, m_, r_, d, n)
        return out
    bmid, bhalf = _corners(bwd, (S1, S2, mid["mean"], mid["r"]), (t1, t2, hm, hr))
    _, bbig = fold_bwd64(S1, S2, mid["mean"], mid["r"], d, n)
    for k in bmid:
        R[k] = Ref(bmid[k], bhalf[k] + 2 * ULP * bbig[k] + TINY)
    if "dalpha" in bmid:            # exactly: the relative bound of S2 (and of r^3) and the ulps of the product -- no floor
        g, r = d["gamma"].astype(f64), mid["r"]
        R["dalpha"] = Ref(bmid["dalpha"], np.abs(g * r ** 3 * d["eps"]) * t2 + 3 * hr / r * np.abs(bmid["dalpha"])
                          + 2 * ULP * np.abs(bmid["dalpha"]) + TINY)
    hk = tuple(bhalf[k] + 2 * ULP * bbig[k] for k in ("ka", "kb", "kc"))
    R["dv"] = apply_ref(c, v, d["dout"], mid["scale"], mid["shift"], bmid["ka"], bmid["kb"], bmid["kc"], hz=hz, hk=hk)
    return R


EVAL_ULPS = 8          # scale and shift of the eval form, and the chain rule back from them, are a handful of fp32 torch operations


@functools.lru_cache(maxsize=4)
def reference_eval(c):
    """ops.bn_elu_pool in eval mode: z = gamma (alpha v + c - running_mean) / sqrt(running_var + eps) + beta, an affine map made by
    fp32 element-wise operations on the host side (EVAL_ULPS ulp of its largest term), then the apply kernels; the gradients come
    back through d scale = sum dz v and d shift = sum dz."""
    d = inputs(c)
    C, v = c.C, d["v"]
    a = d["alpha"].astype(f64) if d["alpha"] is not None else np.ones(C)
    cs = d["cshift"].astype(f64) if d["cshift"] is not None else np.zeros(C)
    g, b, rm, rv = (d[k].astype(f64) for k in ("gamma", "beta", "run_mean", "run_var"))
    r = 1.0 / np.sqrt(rv + d["eps"])
    scale, shift = g * a * r, g * (cs - rm) * r + b
    hs = EVAL_ULPS * ULP * np.abs(scale)
    hsh = EVAL_ULPS * ULP * (np.abs(g * cs * r) + np.abs(g * rm * r) + np.abs(b))
    col = lambda x: np.asarray(x, f64)[None, :, None]
    x = v.astype(f64)
    hz = col(hs) * np.abs(x) + col(hsh)
    R = dict(out=fwd_ref(c, v, scale, shift, hz=hz))
    rs, _, _ = bwd_sums_ref(c, v, d["dout"], scale, shift, np.zeros(C),
                            hz=hz + (K_OUT - 1) * U * (col(np.abs(scale)) * np.abs(x) + col(np.abs(shift))))
    S1, S2, t1, t2 = rs["S1"].ref, rs["S2"].ref, rs["S1"].tol, rs["S2"].tol
    R["dv"] = apply_ref(c, v, d["dout"], scale, shift, scale, np.zeros(C), np.zeros(C), hz=hz, hk=(hs, 0.0, 0.0))
    big = np.abs(S2 * a * r) + np.abs(S1 * cs * r) + np.abs(S1 * rm * r)
    R["dgamma"] = Ref(S2 * a * r + S1 * (cs - rm) * r, t2 * np.abs(a * r) + t1 * np.abs((cs - rm) * r) + EVAL_ULPS * ULP * big + TINY)
    R["dbeta"] = Ref(S1, t1 + EVAL_ULPS * ULP * np.abs(S1) + TINY)
    if d["alpha"] is not None:
        R["dalpha"] = Ref(S2 * g * r, t2 * np.abs(g * r) + EVAL_ULPS * ULP * np.abs(S2 * g * r) + TINY)
        R["dc"] = Ref(S1 * g * r, t1 * np.abs(g * r) + EVAL_ULPS * ULP * np.abs(S1 * g * r) + TINY)
    return R


OP_OUTPUTS = ("out", "dv", "dgamma", "dbeta", "dalpha", "run_mean", "run_var")


# ============================================================================================================ fp32 restatements
DEFECTS = {               # defect -> the plan class it breaks
    "strided_rows": "stats:B>32",
    "tail_threads": "stats:ragged_chain",
    "remainder_dv_zero": "bwd:remainder",
    "dalpha_sign": "fold:dalpha",
    "dalpha_no_eps": "fold:dalpha",
    "biased_running_var": "fold:running",
}
CONTROL_DEFECT = "mean_rounding_in_kb"           # kb from the fp32 mean: must NOT be flagged in the gauss rows


def fma32(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _threads(x):
    """(B, C, T) -> (B, C, chain, 256): element t goes to thread t % 256, pass t // 256 (zeros where there is none)"""
    B, C, T = x.shape
    chain = max(1, cdiv(T, THREADS))
    full = np.zeros((B, C, chain * THREADS), x.dtype)
    full[:, :, :T] = x
    return full.reshape(B, C, chain, THREADS)


def _rows_of_slices(B, defect):
    nsl = stat_slices(B)
    if defect == "strided_rows":
        return np.arange(nsl)                    # every slice takes its first row only
    return np.arange(B)


def expf32(z):
    """__expf: the hardware exp2 of the fp32 product z log2(e)"""
    p = (np.asarray(z, f32) * f32(LOG2E)).astype(f32)
    with np.errstate(under="ignore"):
        return np.exp2(p.astype(f64)).astype(f32)


def elu_grad32(z):
    return np.where(z > 0, f32(1), expf32(np.minimum(z, f32(0)))).astype(f32)


def restate_stats(v, defect=None):
    """(C, 2) doubles: per thread and row an fp32 chain, everything after it in double"""
    B, C, T = v.shape
    x = v.copy()
    if defect == "tail_threads":
        x[:, :, THREADS * (T // THREADS):] = 0
    th = _threads(x)
    fs = np.zeros(th.shape[:2] + (THREADS,), f32)
    fq = np.zeros_like(fs)
    for k in range(th.shape[2]):
        fs = (fs + th[:, :, k]).astype(f32)
        fq = fma32(th[:, :, k], th[:, :, k], fq)
    rows = _rows_of_slices(B, defect)
    return np.stack([fs[rows].astype(f64).sum(axis=(0, 2)), fq[rows].astype(f64).sum(axis=(0, 2))], axis=1)


def restate_fwd(v, scale, shift, P):
    B, C, T = v.shape
    Tp = T // P
    z = fma32(scale[None, :, None], v, shift[None, :, None])
    with np.errstate(over="ignore"):
        e = np.where(z > 0, z, np.expm1(np.minimum(z, f32(0)).astype(f64)).astype(f32)).astype(f32)
    e = e[:, :, :Tp * P].reshape(B, C, Tp, P)
    a = np.zeros((B, C, Tp), f32)
    for i in range(P):
        a = (a + e[..., i]).astype(f32)
    return (a / f32(P)).astype(f32)


def restate_bwd_sums(v, dout, scale, shift, mean, P, defect=None):
    B, C, T = v.shape
    Tp = T // P
    n = Tp * P
    z = fma32(scale[None, :, None], v[:, :, :n], shift[None, :, None])
    invP = f32(1) / f32(P)
    dz = ((elu_grad32(z) * np.repeat(dout, P, axis=2)).astype(f32) * invP).astype(f32)
    vc = (v[:, :, :n] - mean[None, :, None]).astype(f32)
    if defect == "tail_threads":
        dz[:, :, THREADS * (n // THREADS):] = 0
    tdz, tvc = _threads(dz), _threads(vc)
    f1 = np.zeros((B, C, THREADS), f32)
    f2 = np.zeros_like(f1)
    for k in range(tdz.shape[2]):
        f1 = (f1 + tdz[:, :, k]).astype(f32)
        f2 = fma32(tdz[:, :, k], tvc[:, :, k], f2)
    rows = _rows_of_slices(B, defect)
    return f1[rows].astype(f64).sum(axis=(0, 2)), f2[rows].astype(f64).sum(axis=(0, 2))


def restate_apply(v, dout, scale, shift, ka, kb, kc, P, defect=None):
    B, C, T = v.shape
    Tp = T // P
    n = Tp * P
    col = lambda a: np.asarray(a, f32)[None, :, None]
    z = fma32(col(scale), v[:, :, :n], col(shift))
    dz = np.zeros((B, C, T), f32)
    dz[:, :, :n] = ((elu_grad32(z) * np.repeat(dout, P, axis=2)).astype(f32) / f32(P)).astype(f32)
    dv = fma32(col(ka), dz, fma32(col(kc), v, col(kb)))
    if defect == "remainder_dv_zero":
        dv[:, :, n:] = 0
    return dv


def restate_op(c, defect=None, momentum=None, calls=1):
    """ops.bn_elu_pool (training) in kernel order: fp32 where the kernels are fp32, double where they are double"""
    d = inputs(c)
    n = c.B * c.T
    sums = restate_stats(d["v"], defect)
    run = (d["run_mean"], d["run_var"])
    for k in range(1, calls + 1):
        mom = 1.0 / k if momentum == "cumulative" else d["momentum"]
        f, _ = fold_fwd64(sums[:, 0], sums[:, 1], n, d, momentum=mom, defect=defect, run=(run[0].astype(f64), run[1].astype(f64)))
        run = (f["run_mean"].astype(f32), f["run_var"].astype(f32))
    sc, sh = f["scale"].astype(f32), f["shift"].astype(f32)
    out = dict(scale=sc, shift=sh, mean=f["mean"], r=f["r"], run_mean=run[0], run_var=run[1], s=sums[:, 0], q=sums[:, 1])
    out["out"] = restate_fwd(d["v"], sc, sh, c.P)
    S1, S2 = restate_bwd_sums(d["v"], d["dout"], sc, sh, f["mean"].astype(f32), c.P, defect)
    b, _ = fold_bwd64(S1, S2, f["mean"], f["r"], d, n, defect)
    out.update(S1=S1, S2=S2, **{k: x.astype(f32) for k, x in b.items()})
    out["dv"] = restate_apply(d["v"], d["dout"], sc, sh, out["ka"], out["kb"], out["kc"], c.P, defect)
    return out


def restate_direct(c, give):
    """the six entry points on the inputs direct(c) gives them"""
    d = inputs(c)
    n = c.B * c.T
    sums = restate_stats(d["v"])
    f, _ = fold_fwd64(give["sums"][:, 0], give["sums"][:, 1], n, d)
    S1, S2 = restate_bwd_sums(d["v"], d["dout"], give["scale"], give["shift"], give["mean"], c.P)
    b, _ = fold_bwd64(give["bsums"][:, 0], give["bsums"][:, 1], give["fold"][:, 0], give["fold"][:, 1], d, n)
    f32s = lambda o, keep64=(): {k: (x if k in keep64 else x.astype(f32)) for k, x in o.items()}
    return {"ign_chan_stats": dict(s=sums[:, 0], q=sums[:, 1]),
            "ign_bn_fold_fwd": f32s({k: f[k] for k in FOLD_FWD_OUT}, ("mean", "r")),
            "ign_affine_elu_pool_fwd": dict(out=restate_fwd(d["v"], give["scale"], give["shift"], c.P)),
            "ign_bn_elu_pool_bwd_sums": dict(S1=S1, S2=S2),
            "ign_bn_fold_bwd": f32s(b),
            "ign_bn_elu_pool_bwd_apply": dict(dv=restate_apply(d["v"], d["dout"], give["scale"], give["shift"], give["ka"], give["kb"],
                                                               give["kc"], c.P))}


def ratio(got, r):
    """worst |got - ref| / tol (tol 0: 0 if equal, inf if not; NaN counts as inf)"""
    got = np.asarray(got, f64).reshape(r.ref.shape)
    diff = np.abs(got - r.ref)
    diff = np.where(np.isnan(diff), np.inf, diff)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(r.tol > 0, diff / np.where(r.tol > 0, r.tol, 1.0), np.where(diff == 0, 0.0, np.inf))
    return float(q.max()) if q.size else 0.0
