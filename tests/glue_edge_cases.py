"""The small kernels that stitch the training step together -- the class head, the two SBM regularisers (csrc/ign_head.hip) and the
FCN BatchNorm / pool / bound glue (csrc/ign_bn.hip) -- at every edge of their launch arithmetic: the arithmetic restated in Python,
the case tables built from its branch points, float64 references, fp32 restatements in kernel order, and the tolerances.

Tolerance rule.  u = 2^-24.  An output that is a sum is held to  d * u * sum |a_i||b_i|  +  1 ulp of the result, the sum taken in
float64 over the terms of that one output and d the longest serial chain of fp32 additions on its path (`plan_*` below), never
above D_CAP = 96 -- a longer chain is held to 96, which is the tighter bound.  An elementwise output is held to a stated number of
ulps of its largest term.  Every case also runs in the `exact` regime: small integers times powers of two, sized so that no fp32 sum
rounds; there d = 0, and what has no elementwise rounding must equal float64 exactly.  The finalize outputs take the bounds of s and
q through the float64 formulas (evaluated at the interval ends) plus 2 ulp.  The diversity and regulariser kernels keep the suite's
bounds (loss 1e-5 relative, gradient 1e-4 of its maximum), which tests/test_glue_edges_host.py shows an fp32 restatement meets with
4x headroom in every regime.  Nothing here is read from a kernel's output."""
import functools
import math

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
ULP = 2.0 ** -23                  # 1 ulp of x is at most ULP * |x|
TINY = 2.0 ** -126                # below the smallest normal an fp32 value has no relative precision
D_CAP = 96
IGN_E_ARG, IGN_E_UNSUP, IGN_E_TOOBIG = -1001, -1002, -1003

# constants of csrc/ign_head.hip and csrc/ign_bn.hip (tests/test_glue_edges_host.py parses the sources and compares)
HEAD_NMAX, HEAD_NMAX_ABI = 16, 256
HEAD_LONG_F, HEAD_F_SLICE, HEAD_B_GROUPS, HEAD_X_BLOCK, HEAD_LDS_G_BYTES = 32768, 32, 8, 1024, 40 * 1024
BN_CH, BN_SL, BN_FLUSH = 8, 128, 64
POOL_ROWS, APPLY_ROWS = 128, 64
AMM_MAX, SCAN_LMAX = 16, 8
DIV_KMAX, REG_GMAX, REG_BLOCK = 16, 8, 1024
REG_TICKET_WORD, REG_PARTS_WORD = 0, 4
DIV_EPS = 1e-6

LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-4          # diversity / regulariser: the bounds the suite already uses


def cdiv(a, b):
    return -(-a // b)


class Case:
    def __init__(self, entry, regime, **p):
        self.entry, self.regime, self.p = entry, regime, p
        self.name = "-".join(f"{k}{'x'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in p.items())
        self.id = f"{entry}-{self.name}-{regime}"

    def __getattr__(self, k):
        try:
            return self.__dict__["p"][k]
        except KeyError:
            raise AttributeError(k)

    def __repr__(self):
        return self.id


class Ref:
    """ref (float64), tol (float64, same shape; 0 = must be equal), d = the chain the bound was made with"""

    def __init__(self, ref, tol, d=0, chain=None):
        self.ref = np.asarray(ref, f64)
        self.tol = np.broadcast_to(np.asarray(tol, f64), self.ref.shape).copy()
        self.d, self.chain = d, d if chain is None else chain


def sum_bound(ref, cond, chain, exact):
    """d u sum|a||b| + 1 ulp; the exact regime: 0"""
    d = min(chain, D_CAP)
    if exact:
        return Ref(ref, 0.0, 0, chain)
    return Ref(ref, d * U * cond + ULP * np.abs(ref) + TINY, d, chain)


def _rng(case):
    import zlib
    return np.random.default_rng(zlib.crc32(case.id.encode()))


def _ints(rng, lo, hi, *shape):
    return rng.integers(lo, hi + 1, size=shape).astype(f32)


def fma32(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def seqsum32(x, axis):
    """fp32 sum in ascending order along `axis` (np.cumsum is serial)"""
    x = np.asarray(x, f32)
    if x.shape[axis] == 0:
        return np.zeros(np.delete(x.shape, axis), f32)
    return np.take(np.cumsum(x, axis=axis, dtype=f32), -1, axis=axis)


def butterfly64(v):
    """v (..., 64) -> the value every lane holds after the xor butterfly 32, 16, ... 1"""
    v = np.asarray(v, f32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ o]).astype(f32)
    return v[..., 0]


# ===================================================================================================================== head forward
def plan_head_fwd(F, N, B, ldx, bias):
    nthr = 1024 if F >= HEAD_LONG_F else 256
    f4 = F // 4
    steps = cdiv(f4, nthr)
    waves = nthr // 64
    cls = {f"fwd:nthr{nthr}", "fwd:bias" if bias else "fwd:nobias", "fwd:ldx=F" if ldx == F else "fwd:ldx>F",
           "fwd:one_step" if steps == 1 else "fwd:many_steps", f"fwd:N{N}", f"fwd:B{B}", f"fwd:F{F}"}
    if f4 < nthr:
        cls.add("fwd:idle_threads")
    if f4 % nthr:
        cls.add("fwd:ragged_last_step")
    if f4 < 64:
        cls.add("fwd:idle_waves")
    return dict(route=f"head_fwd_kernel<{'true' if N > HEAD_NMAX else 'false'}> {nthr} threads", nthr=nthr, steps=steps, waves=waves,
                chain=steps * 4 + 6 + waves + 1, classes=cls, wide=N > HEAD_NMAX)


HEAD_FWD_F = (4, 8, 1020, 1024, 1028, 32764, 32768)
HEAD_FWD_N = (1, 2, 3, 15, 16)


def _head_fwd_cases():
    out, i = [], 0
    for F in HEAD_FWD_F:
        for N in HEAD_FWD_N:
            out.append(dict(F=F, N=N, B=(1, 3)[i % 2], pad=(0, 4, 8)[i % 3], bias=int(i % 4 < 2)))
            i += 1
    out.append(dict(F=1028, N=17, B=3, pad=4, bias=1))            # one row past HEAD_NMAX: the table straddles the switch
    return [Case("head_fwd", r, **p) for p in out for r in ("gauss", "exact")]


def inputs_head_fwd(c):
    g, ex = _rng(c), c.regime == "exact"
    ldx = c.F + c.pad
    X = np.full((c.B, ldx), np.nan, f32)
    X[:, :c.F] = _ints(g, -3, 3, c.B, c.F) if ex else g.standard_normal((c.B, c.F)).astype(f32)
    W = _ints(g, -2, 2, c.N, c.F) if ex else g.standard_normal((c.N, c.F)).astype(f32)
    bias = (_ints(g, -4, 4, c.N) if ex else g.standard_normal(c.N).astype(f32)) if c.bias else None
    return dict(X=X, W=W, bias=bias)


def reference_head_fwd(c, d):
    pl = plan_head_fwd(c.F, c.N, c.B, c.F + c.pad, c.bias)
    x, w = d["X"][:, :c.F].astype(f64), d["W"].astype(f64)
    b = d["bias"].astype(f64) if c.bias else np.zeros(c.N)
    return dict(out=sum_bound(x @ w.T + b, np.abs(x) @ np.abs(w).T + np.abs(b), pl["chain"], c.regime == "exact"))


def restate_head_fwd(c, d, defect=None):
    """fp32 in kernel order; defect 'last_wave': the final sum stops one wave early"""
    pl = plan_head_fwd(c.F, c.N, c.B, c.F + c.pad, c.bias)
    nthr, steps, waves = pl["nthr"], pl["steps"], pl["waves"]
    x, W = d["X"][:, :c.F], d["W"]
    p = (x[:, None, :] * W[None, :, :]).astype(f32).reshape(c.B, c.N, c.F // 4, 4)
    s4 = (((p[..., 0] + p[..., 1]).astype(f32) + p[..., 2]).astype(f32) + p[..., 3]).astype(f32)
    full = np.zeros((c.B, c.N, steps * nthr), f32)
    full[..., :c.F // 4] = s4
    acc = seqsum32(full.reshape(c.B, c.N, steps, nthr), 2)
    red = butterfly64(acc.reshape(c.B, c.N, waves, 64))
    t = seqsum32(red[..., :waves - 1] if defect == "last_wave" else red, 2)
    return dict(out=(t + (d["bias"] if c.bias else f32(0))).astype(f32))


# ===================================================================================================================== head backward
def plan_head_bwd(B, F, N, mode, gbias, add):
    gsn = HEAD_NMAX if N > HEAD_NMAX else N
    if B * gsn * 4 > HEAD_LDS_G_BYTES:
        return dict(route="IGN_E_TOOBIG", refused=IGN_E_TOOBIG, classes={"bwd:toobig"}, chain={})
    per = cdiv(B, HEAD_B_GROUPS)
    b0 = [g * per for g in range(HEAD_B_GROUPS)]
    live = [x for x in b0 if x < B]
    nfb, nxb = cdiv(F, HEAD_F_SLICE), cdiv(F // 4, 256)
    lds = (B * gsn + HEAD_B_GROUPS * HEAD_NMAX * HEAD_F_SLICE) * 4
    cls = {f"bwd:{mode}", f"bwd:{mode}:{'gbias' if gbias else 'nogbias'}", f"bwd:add_{add}", f"bwd:B{B}", f"bwd:F{F}",
           "bwd:per1" if per == 1 else "bwd:per>1"}
    if any(x > B for x in b0):
        cls.add("bwd:empty_group_b0>B")
    if any(x == B for x in b0):
        cls.add("bwd:empty_group_b0=B")
    if len(live) == HEAD_B_GROUPS and B % HEAD_B_GROUPS:
        cls.add("bwd:short_last_group")
    if F % HEAD_F_SLICE:
        cls.add("bwd:ragged_f_slice")
    if F < HEAD_F_SLICE:
        cls.add("bwd:one_short_slice")
    if nxb > 1:
        cls.add("bwd:two_x_blocks")
    if (F // 4) % 256:
        cls.add("bwd:ragged_x_block")
    if B * gsn * 4 > HEAD_LDS_G_BYTES - 16:
        cls.add("bwd:lds_at_limit")
    grid = dict(xw=nfb + nxb * B, x=nxb * B, w=nfb)[mode]
    chain = {}
    if "x" in mode:
        chain["gX"] = N
    if "w" in mode:
        chain["gW"] = per + HEAD_B_GROUPS + (2 if add != "none" else 0)
        if gbias:
            chain["gbias"] = B
    return dict(route=f"head_bwd_{mode}_kernel<false> grid {grid}, {lds} B LDS", per=per, live=len(live), nfb=nfb, nxb=nxb, lds=lds,
                grid=grid, chain=chain, classes=cls, refused=0)


HEAD_BWD_B = (1, 7, 8, 9, 16, 17, 65)
HEAD_BWD_F = (4, 28, 32, 36, 1020, 1024, 1028)


def _head_bwd_cases():
    rows, i = [], 0
    for B in HEAD_BWD_B:
        for F in HEAD_BWD_F:
            rows.append(dict(B=B, F=F, N=(3, 16, 1, 15, 2)[i % 5], mode=("xw", "x", "w")[i % 3], gbias=(i // 3) % 2,
                             add=("none", "scaled", "unscaled")[(i // 6) % 3], pad=(0, 4, 8)[(i // 2) % 3]))
            i += 1
    rows.append(dict(B=640, F=36, N=16, mode="xw", gbias=1, add="scaled", pad=4))           # 40960 bytes of g: the limit
    rows.append(dict(B=3413, F=4, N=3, mode="w", gbias=1, add="unscaled", pad=0))           # 40956 bytes
    return [Case("head_bwd", r, **p) for p in rows for r in ("gauss", "exact")]


HEAD_BWD_TOOBIG = [dict(B=641, F=36, N=16), dict(B=3414, F=4, N=3)]


def inputs_head_bwd(c):
    rng, ex = _rng(c), c.regime == "exact"
    ldx = c.F + c.pad
    draw = (lambda lo, hi, *s: _ints(rng, lo, hi, *s)) if ex else (lambda lo, hi, *s: rng.standard_normal(s).astype(f32))
    X = np.full((c.B, ldx), np.nan, f32)
    X[:, :c.F] = draw(-3, 3, c.B, c.F)
    d = dict(g=draw(-2, 2, c.B, c.N), X=X, W=draw(-2, 2, c.N, c.F))
    if c.add != "none":
        d["add"] = draw(-5, 5, c.N, c.F)
        if c.add == "scaled":
            d["scale"] = np.array([0.5 if ex else 0.37], f32)
    return d


def reference_head_bwd(c, d):
    pl, ex = plan_head_bwd(c.B, c.F, c.N, c.mode, c.gbias, c.add), c.regime == "exact"
    g, x, w = d["g"].astype(f64), d["X"][:, :c.F].astype(f64), d["W"].astype(f64)
    out = {}
    if "x" in c.mode:
        out["gX"] = sum_bound(g @ w, np.abs(g) @ np.abs(w), pl["chain"]["gX"], ex)
    if "w" in c.mode:
        extra = (float(d["scale"][0]) if c.add == "scaled" else 1.0) * d["add"].astype(f64) if c.add != "none" else 0.0
        out["gW"] = sum_bound(g.T @ x + extra, np.abs(g).T @ np.abs(x) + np.abs(extra), pl["chain"]["gW"], ex)
        if c.gbias:
            out["gbias"] = sum_bound(g.sum(0), np.abs(g).sum(0), pl["chain"]["gbias"], ex)
    return out


def restate_head_bwd(c, d, defect=None):
    """fp32 in kernel order (the weight gradient and gbias); defect 'last_group': with B % 8 != 0 the last non-empty batch group is
    left out of the combination"""
    pl = plan_head_bwd(c.B, c.F, c.N, c.mode, c.gbias, c.add)
    g, x = d["g"], d["X"][:, :c.F]
    per, parts = pl["per"], []
    for grp in range(HEAD_B_GROUPS):
        acc = np.zeros((c.N, c.F), f32)
        for b in range(grp * per, min(c.B, grp * per + per)):
            acc = fma32(g[b][:, None], x[b][None, :], acc)
        parts.append(acc)
    if defect == "last_group" and c.B % HEAD_B_GROUPS:
        parts[pl["live"] - 1] = np.zeros((c.N, c.F), f32)
    s = seqsum32(np.stack(parts), 0)
    if c.add != "none":
        sc = d["scale"][0] if c.add == "scaled" else f32(1)
        s = (s + (sc * d["add"]).astype(f32)).astype(f32)
    out = dict(gW=s)
    if c.gbias:
        out["gbias"] = seqsum32(g, 0)
    return out


# ===================================================================================================================== BatchNorm finalize
def plan_bn_sum(nparts, C):
    per = cdiv(nparts, BN_SL)
    used = cdiv(nparts, per)
    last = nparts - (used - 1) * per
    cls = {f"fin:C{C}", f"fin:nparts{nparts}", "fin:per1" if per == 1 else "fin:per>1"}
    if used < BN_SL:
        cls.add("fin:empty_slices")
    if last < per:
        cls.add("fin:short_last_slice")
    if per == BN_FLUSH:
        cls.add("fin:flush_at_slice_end")
    if per == BN_FLUSH + 1:
        cls.add("fin:flush_one_before_slice_end")
    if last == BN_FLUSH and per > BN_FLUSH:
        cls.add("fin:flush_at_short_slice_end")
    if per > BN_FLUSH:
        cls.add("fin:flush_inside_slice")
    if C % BN_CH:
        cls.add("fin:ragged_channel_block")
    if C > BN_CH:
        cls.add("fin:many_channel_blocks")
    if C < BN_CH:
        cls.add("fin:one_short_channel_block")
    return dict(route=f"bn_sum_partials grid {cdiv(C, BN_CH)}, per {per}, {used} slices", per=per, used=used, last=last,
                chain=max(min(per, BN_FLUSH) - 1, 0), classes=cls)


FIN_NPARTS = (1, 2, 127, 128, 129, 257, 8192, 8193, 8320, 8321)
FIN_C = (1, 7, 8, 9, 1024)


def _finalize_cases():
    rows = []
    for i, n in enumerate(FIN_NPARTS):
        rows.append(dict(nparts=n, C=(1, 7, 8, 9)[i % 4], rpp=4, run=i % 2))
        rows.append(dict(nparts=n, C=(9, 8, 1, 7)[i % 4], rpp=4, run=1 - i % 2))
    rows += [dict(nparts=n, C=1024, rpp=4, run=i % 2) for i, n in enumerate((1, 2, 129, 257))]
    rows += [dict(nparts=1, C=9, rpp=1, run=1), dict(nparts=1, C=8, rpp=1, run=0)]                      # R = 1
    return [Case(e, r, **p) for p in rows for r in ("gauss", "exact") for e in ("bn_finalize_fwd", "bn_finalize_bwd")]


FIN_EPS, FIN_MOM = f32(1e-5), {"gauss": f32(0.1), "exact": f32(0.125)}


def fin_mean_ratio(chain):
    """largest |mean| / sigma of {4, 2, 1, 0.5, 0.25, 0} that keeps the relative invstd tolerance of a chain under 0.8e-5:
    d invstd / invstd = dvar / (2 var), dvar <= d u (E y^2 + 2 |m| E|y|) <= d u sigma^2 (1 + r^2 + 2 r (r + 0.8))"""
    for r in (4.0, 2.0, 1.0, 0.5, 0.25, 0.0):
        if 0.5 * chain * U * (1 + r * r + 2 * r * (r + 0.8)) <= 0.8e-5:
            return r
    raise AssertionError(chain)


@functools.lru_cache(maxsize=None)
def _inputs_finalize(nparts, C, rpp, regime):
    """the partials are shared by the forward and the backward finalize of a row"""
    c = Case("bn_finalize", regime, nparts=nparts, C=C, rpp=rpp)
    rng = _rng(c)
    pl = plan_bn_sum(nparts, C)
    if regime == "exact":
        sign = np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
        part = np.empty((nparts, 2, C), f32)
        part[:, 0] = _ints(rng, 1, 3, nparts, C) * sign
        part[:, 1] = _ints(rng, 4 * rpp, 12 * rpp, nparts, C)
        if rpp > 1:                      # channel 0 is constant (y = 1.5 on every row) with q a shade low: q / R - m * m = -2^-14
            part[:, 0, 0], part[:, 1, 0] = 1.5 * rpp, 2.25 * rpp - 2.0 ** -12
        gamma = np.where(np.arange(C) % 3 == 0, -2.0, 0.5).astype(f32)
        beta, rm, rv = _ints(rng, -3, 3, C), _ints(rng, -3, 3, C), _ints(rng, 1, 4, C)
    else:
        ratio = fin_mean_ratio(pl["chain"])
        sigma = rng.uniform(0.5, 2.0, C)
        mean = rng.uniform(-1, 1, C) * ratio * sigma
        part = np.empty((nparts, 2, C), f32)
        step = max(1, 65536 // (C * rpp))
        for i in range(0, nparts, step):
            y = mean + sigma * rng.standard_normal((min(step, nparts - i), rpp, C))
            part[i:i + step, 0], part[i:i + step, 1] = y.sum(1), (y * y).sum(1)
        gamma, beta = rng.standard_normal(C).astype(f32), rng.standard_normal(C).astype(f32)
        rm, rv = rng.standard_normal(C).astype(f32), rng.uniform(0.5, 2, C).astype(f32)
    return dict(part=part, gamma=gamma, beta=beta, run_mean=rm, run_var=rv)


def inputs_finalize(c):
    d = dict(_inputs_finalize(c.nparts, c.C, c.rpp, c.regime))
    if not c.run:
        d["run_mean"] = d["run_var"] = None
    return d


def _fin_formulas(s, q, R, d, mom):
    eps = float(FIN_EPS)
    m = s / R
    var = np.maximum(q / R - m * m, 0.0)
    inv = 1.0 / np.sqrt(var + eps)
    a = d["gamma"].astype(f64) * inv
    out = dict(a=a, b=d["beta"].astype(f64) - a * m, mean=m, invstd=inv)
    big = dict(a=np.abs(a), b=np.maximum(np.abs(d["beta"]), np.abs(a * m)), mean=np.abs(m), invstd=inv)
    if d["run_mean"] is not None:
        unb = var * R / (R - 1) if R > 1 else var
        out["run_mean"] = (1 - mom) * d["run_mean"] + mom * m
        out["run_var"] = (1 - mom) * d["run_var"] + mom * unb
        big["run_mean"] = np.maximum(np.abs((1 - mom) * d["run_mean"]), np.abs(mom * m))
        big["run_var"] = np.maximum(np.abs((1 - mom) * d["run_var"]), np.abs(mom * unb))
    return out, big


def reference_finalize(c, d):
    pl, ex = plan_bn_sum(c.nparts, c.C), c.regime == "exact"
    p = d["part"].astype(f64)
    s, q = p[:, 0].sum(0), p[:, 1].sum(0)
    chain = pl["chain"]
    dd = 0 if ex else min(chain, D_CAP)
    ts, tq = dd * U * np.abs(p[:, 0]).sum(0), dd * U * np.abs(p[:, 1]).sum(0)
    if c.entry == "bn_finalize_bwd":
        return dict(dbeta=Ref(s, ts + ULP * np.abs(s) + TINY, dd, chain), dgamma=Ref(q, tq + ULP * np.abs(q) + TINY, dd, chain))
    R, mom = c.nparts * c.rpp, float(FIN_MOM[c.regime])
    mid, big = _fin_formulas(s, q, R, d, mom)
    half = {k: np.zeros(c.C) for k in mid}
    for ds in (-1, 1):
        for dq in (-1, 1):
            corner, _ = _fin_formulas(s + ds * ts, q + dq * tq, R, d, mom)
            for k in mid:
                half[k] = np.maximum(half[k], np.abs(corner[k] - mid[k]))
    out = {k: Ref(mid[k], half[k] + 2 * ULP * big[k] + TINY, dd, chain) for k in mid}
    if ex:            # s and q are exact: mean and invstd are one rounding of a float64 value, a = gamma * invstd with gamma a power of two
        inv32 = mid["invstd"].astype(f32)
        out.update(mean=Ref(mid["mean"].astype(f32), 0.0, 0, chain), invstd=Ref(inv32, 0.0, 0, chain),
                   a=Ref((d["gamma"] * inv32).astype(f32), 0.0, 0, chain))
    return out


def restate_bn_sum(part, defect=None):
    """(s, q) float64 per channel in kernel order; defect 'short_slice': a last slice shorter than the others is forgotten"""
    nparts, _, C = part.shape
    pl = plan_bn_sum(nparts, C)
    per, tot = pl["per"], np.zeros((2, C), f64)
    for sl in range(BN_SL):
        i0, i1 = sl * per, min(nparts, sl * per + per)
        if i1 <= i0 or (defect == "short_slice" and i1 - i0 < per):
            continue
        acc = np.zeros((2, C), f64)
        for j in range(i0, i1, BN_FLUSH):
            acc += seqsum32(part[j:min(i1, j + BN_FLUSH)], 0).astype(f64)
        tot += acc
    return tot[0], tot[1]


# ===================================================================================================================== affine eval
AFFINE_C = (1, 255, 256, 257)


def inputs_affine(c):
    rng = _rng(c)
    if c.regime == "exact":                          # var + eps = 0.25 needs eps of its own: the test passes eps = 0 and var = 4^k
        return dict(run_mean=_ints(rng, -3, 3, c.C), run_var=f32(4.0) ** _ints(rng, -2, 2, c.C), gamma=_ints(rng, -3, 3, c.C),
                    beta=_ints(rng, -3, 3, c.C), eps=f32(0))
    return dict(run_mean=rng.standard_normal(c.C).astype(f32), run_var=rng.uniform(0.0, 2, c.C).astype(f32),
                gamma=rng.standard_normal(c.C).astype(f32), beta=rng.standard_normal(c.C).astype(f32), eps=FIN_EPS)


def reference_affine(c, d):
    """4 ulp of the largest term; exact regime: equal"""
    m, v, g, b = (d[k].astype(f64) for k in ("run_mean", "run_var", "gamma", "beta"))
    inv = 1.0 / np.sqrt(v + float(d["eps"]))
    a = g * inv
    k = 0.0 if c.regime == "exact" else 4 * ULP
    return dict(a=Ref(a, k * np.abs(a)), b=Ref(b - a * m, k * np.maximum(np.abs(b), np.abs(a * m))), mean=Ref(m, 0.0),
                invstd=Ref(inv, k * inv))


# ===================================================================================================================== pool forward / backward
def plan_pool(C, T, rows=None):
    """rows: the rows one block walks (the forward: T; the backward: <= POOL_ROWS)"""
    if C <= 0 or C % 4 or C > 1024:
        return dict(route="IGN_E_ARG", refused=IGN_E_ARG)
    rows = T if rows is None else rows
    c4 = C // 4
    rif = 256 // c4
    idle = 256 - rif * c4
    steps = cdiv(rows, rif)
    cls = {f"pool:C{C}", f"pool:rif{rif}", "pool:idle_threads" if idle else "pool:no_idle_threads"}
    cls.add("pool:T<rif" if rows < rif else "pool:T=rif" if rows == rif else "pool:T=k*rif+1" if rows % rif == 1 else "pool:T>rif")
    if rows == rif - 1:
        cls.add("pool:T=rif-1")
    if C > 256:
        cls.add("pool:several_columns_per_thread")
    return dict(route=f"c4 {c4}, rif {rif}, {idle} idle threads, {steps} rows per thread", c4=c4, rif=rif, idle=idle, steps=steps,
                chain=steps + min(rows, rif) + 2, lds=rif * C * 4, classes=cls, refused=0)


POOL_C = (4, 12, 24, 128, 256, 260, 1024)
POOL_RIF = (256, 85, 42, 8, 4, 3, 1)
POOL_IDLE = (0, 1, 4, 0, 0, 61, 0)
POOL_HEAD_N = (1, 3, 4, 5, 16, 17, 40)
POOL_REFUSED_C = (6, 1028)


def _pool_fwd_cases():
    rows, i = [], 0
    for C, rif in zip(POOL_C, POOL_RIF):
        for T in sorted({t for t in (1, rif - 1, rif, rif + 1, 2 * rif + 1) if t > 0}):
            head = i % 3 != 2
            rows.append(dict(C=C, T=T, B=(1, 3)[i % 2], N=POOL_HEAD_N[i % 7] if head else 0, bias=int(head and i % 4 < 2)))
            i += 1
    return [Case("bn_relu_pool_fwd", r, **p) for p in rows for r in ("gauss", "exact", "negative")]


def _pool_abym(c, rng):
    """a, b, y (and mean, invstd) of a pool case"""
    C = c.C
    if c.regime == "gauss":
        a, b = rng.standard_normal(C).astype(f32), (0.3 * rng.standard_normal(C)).astype(f32)
        y = rng.standard_normal((c.B, c.T, C)).astype(f32)
        return a, b, y, rng.standard_normal(C).astype(f32), rng.uniform(0.5, 2, C).astype(f32)
    a = np.where(np.arange(C) % 2 == 0, 1.0, -2.0).astype(f32)
    if c.regime == "negative":                       # a y + b <= -1 everywhere
        y = _ints(rng, 1, 6, c.B, c.T, C) * np.sign(-a)
        return a, np.full(C, -1, f32), y.astype(f32), np.zeros(C, f32), np.ones(C, f32)
    b = _ints(rng, -2, 2, C)
    y = _ints(rng, -4, 4, c.B, c.T, C)
    zero = rng.random((c.B, c.T, C)) < 0.25            # a quarter of the pre-activations exactly 0: y = -b / a (a = 1: -b; a = -2: b / 2)
    y = np.where(zero, np.where(a > 0, -b, b / 2), y).astype(f32)
    return a, b, y, _ints(rng, -2, 2, C), (f32(2.0) ** _ints(rng, -1, 1, C)).astype(f32)


def inputs_pool_fwd(c):
    rng = _rng(c)
    a, b, y, _, _ = _pool_abym(c, rng)
    d = dict(y=y, a=a, b=b)
    if c.N:
        ex = c.regime != "gauss"
        d["W"] = _ints(rng, -2, 2, c.N, c.C) if ex else rng.standard_normal((c.N, c.C)).astype(f32)
        d["bias"] = (_ints(rng, -4, 4, c.N) if ex else rng.standard_normal(c.N).astype(f32)) if c.bias else None
    return d


def reference_pool_fwd(c, d):
    """pooled only; the logits are held to the float64 product of the kernel's own pooled row (`reference_pool_logits`)"""
    pl, ex = plan_pool(c.C, c.T), c.regime != "gauss"
    v = np.maximum(d["a"].astype(f64) * d["y"].astype(f64) + d["b"].astype(f64), 0.0)
    ref = v.sum(1) / c.T
    if ex:                                            # the sum is exact, the division rounds once: equal to the bit
        return dict(pooled=Ref(ref.astype(f32), 0.0, 0, pl["chain"]))
    return dict(pooled=sum_bound(ref, v.sum(1) / c.T, pl["chain"], False))


def plan_pool_logits(C):
    return dict(chain=cdiv(C, 64) + 6 + 1)


def reference_pool_logits(c, d, pooled):
    """exact regime: pooled = integer / T is not an integer, so the products round: the sum bound holds in every regime"""
    p, w = np.asarray(pooled, f64), d["W"].astype(f64)
    b = d["bias"].astype(f64) if c.bias else np.zeros(c.N)
    return sum_bound(p @ w.T + b, np.abs(p) @ np.abs(w).T + np.abs(b), plan_pool_logits(c.C)["chain"], False)


def restate_pool_fwd(c, d, defect=None):
    """fp32 in kernel order; defect 'tail_rows': the rows past rif * floor(T / rif) are forgotten"""
    pl = plan_pool(c.C, c.T)
    rif, steps = pl["rif"], pl["steps"]
    v = np.maximum(fma32(d["a"], d["y"], d["b"]), f32(0))
    if defect == "tail_rows":
        v = v.copy()
        v[:, rif * (c.T // rif):] = 0
    full = np.zeros((c.B, steps * rif, c.C), f32)
    full[:, :c.T] = v
    s = seqsum32(full.reshape(c.B, steps, rif, c.C), 1)
    return dict(pooled=(seqsum32(s, 1) / f32(c.T)).astype(f32))


POOL_BWD_T = (1, 127, 128, 129, 257)


def _pool_bwd_cases():
    rows, i = [], 0
    for C in POOL_C:
        for T in POOL_BWD_T:
            rows.append(dict(C=C, T=T, B=(1, 3)[i % 2] if C * T < 200000 else 1, part=int(i % 3 != 1)))
            i += 1
    return [Case("bn_relu_pool_bwd", r, **p) for p in rows for r in ("gauss", "exact")]


def plan_pool_bwd(C, T, B):
    nb = cdiv(T, POOL_ROWS)
    last = T - (nb - 1) * POOL_ROWS
    pl = plan_pool(C, T, min(T, POOL_ROWS))
    cls = set(pl["classes"]) | {f"poolbwd:T{T}", "poolbwd:one_block" if nb == 1 else "poolbwd:many_blocks"}
    if last < POOL_ROWS:
        cls.add("poolbwd:short_last_block")
    if last == 1 and nb > 1:
        cls.add("poolbwd:one_row_last_block")
    return dict(route=f"grid ({nb}, {B}), " + pl["route"], nblocks=nb, parts=B * nb, chain=pl["chain"], classes=cls, rif=pl["rif"])


def inputs_pool_bwd(c):
    rng = _rng(c)
    a, b, y, mean, invstd = _pool_abym(c, rng)
    gp = _ints(rng, -3, 3, c.B, c.C) if c.regime == "exact" else rng.standard_normal((c.B, c.C)).astype(f32)
    return dict(y=y, gpool=gp, a=a, b=b, mean=mean, invstd=invstd)


def reference_pool_bwd(c, d):
    """g: 2 ulp (1 / T and the product round); with T a power of two and integer gpool it is exact"""
    mask = d["a"].astype(f64) * d["y"].astype(f64) + d["b"].astype(f64) > 0
    g = np.where(mask, d["gpool"].astype(f64)[:, None, :] / c.T, 0.0)
    exact = c.regime == "exact" and c.T & (c.T - 1) == 0
    return dict(g=Ref(g, 0.0 if exact else 2 * ULP * np.abs(g)))


def reference_pool_bwd_sums(c, d, g):
    """dbeta, dgamma after ign_bn_finalize_bwd over the kernel's partials, against float64 sums over the kernel's OWN g: what is on
    trial is the summation (pool partials, then the finalize).  Exact where the addends are (T a power of two)."""
    pl = plan_pool_bwd(c.C, c.T, c.B)
    fin = plan_bn_sum(pl["parts"], c.C)
    g = np.asarray(g, f64)
    yhat = (d["y"].astype(f64) - d["mean"].astype(f64)) * d["invstd"].astype(f64)
    exact = c.regime == "exact" and c.T & (c.T - 1) == 0
    t0, t1 = g.reshape(-1, c.C), (g * yhat).reshape(-1, c.C)
    chain = pl["chain"] + fin["chain"]
    return dict(dbeta=sum_bound(t0.sum(0), np.abs(t0).sum(0), chain, exact), dgamma=sum_bound(t1.sum(0), np.abs(t1).sum(0), chain + 3, exact))


# ===================================================================================================================== bn_bwd_apply
APPLY_PADS = (0, 1, 3, 4)
APPLY_ROWSETS = (63, 64, 65, 129)
_APPLY_64 = {0: (4, 16), 1: (16, 2), 3: (8, 2), 4: (4, 8)}           # rows = 64 with R = B T a power of two


def apply_shape(rows, pad):
    if rows == 64:
        return _APPLY_64[pad]
    for B in (3, 5, 7, 1):
        if rows % B == 0 and rows // B - 2 * pad >= 1:
            return B, rows // B - 2 * pad
    raise AssertionError((rows, pad))


def plan_apply(B, T, C, pad):
    if C <= 0 or C % 4 or C > 1024:
        return dict(route="IGN_E_ARG", refused=IGN_E_ARG)
    c4 = C // 4
    rif = 256 // c4
    rows = B * (T + 2 * pad)
    nb = cdiv(rows, APPLY_ROWS)
    cls = {f"apply:pad{pad}", f"apply:rows{rows}", f"apply:C{C}", "apply:one_block" if nb == 1 else "apply:many_blocks"}
    if rows % APPLY_ROWS:
        cls.add("apply:short_last_block")
    if 256 % c4:
        cls.add("apply:dead_lanes_in_last_wave")
    return dict(route=f"grid {nb}, rif {rif}, {256 - rif * c4} idle threads", rows=rows, nblocks=nb, rif=rif, classes=cls, refused=0)


def _apply_cases():
    rows, i = [], 0
    for pad in APPLY_PADS:
        for r in APPLY_ROWSETS:
            for tr in (1, 0):
                B, T = apply_shape(r, pad)
                rows.append(dict(B=B, T=T, C=(4, 12, 24, 128, 260, 1024)[i % 6], pad=pad, tr=tr, slot=("none", "zero", "above")[(i // 2) % 3]))
                i += 1
    for C in (12, 24, 260):                                                             # the shuffle after the early return
        for j, slot in enumerate(("zero", "above")):
            B, T = apply_shape(APPLY_ROWSETS[j + 1], 1)
            rows.append(dict(B=B, T=T, C=C, pad=1, tr=1 - j, slot=slot))
    return [Case("bn_bwd_apply", r, **p) for p in rows for r in ("gauss", "exact")]


def inputs_apply(c):
    rng, C = _rng(c), c.C
    if c.regime == "exact":
        d = dict(g=_ints(rng, -3, 3, c.B, c.T, C), y=_ints(rng, -3, 3, c.B, c.T, C), a=(f32(2.0) ** _ints(rng, -1, 1, C)).astype(f32),
                 mean=_ints(rng, -2, 2, C), invstd=(f32(2.0) ** _ints(rng, -1, 1, C)).astype(f32), dbeta=_ints(rng, -3, 3, C),
                 dgamma=_ints(rng, -3, 3, C))
    else:
        n = lambda *s: rng.standard_normal(s).astype(f32)
        d = dict(g=n(c.B, c.T, C), y=n(c.B, c.T, C), a=n(C), mean=n(C), invstd=rng.uniform(0.5, 2, C).astype(f32),
                 dbeta=(n(C) * math.sqrt(c.B * c.T)).astype(f32), dgamma=(n(C) * math.sqrt(c.B * c.T)).astype(f32))
    if not c.tr:
        for k in ("y", "mean", "invstd", "dbeta", "dgamma"):
            d[k] = None
    return d


def reference_apply(c, d):
    """dyp (B, T + 2 pad, C): 4 ulp of the largest term inside, exactly 0 on the pad rows.  Exact regime: equal where every
    coefficient is exact (eval mode, or R a power of two)."""
    R = c.B * c.T
    a, g = d["a"].astype(f64), d["g"].astype(f64)
    val, big = a * g, np.abs(a * g)
    if c.tr:
        y, m, iv, db, dg = (d[k].astype(f64) for k in ("y", "mean", "invstd", "dbeta", "dgamma"))
        val = a * (g - (db + (y - m) * iv * dg) / R)
        for t in (a * iv * dg * y / R, a * db / R + 0 * y, a * m * iv * dg / R + 0 * y):
            big = np.maximum(big, np.abs(t))
    exact = c.regime == "exact" and (not c.tr or R & (R - 1) == 0)
    ref, tol = np.zeros((c.B, c.T + 2 * c.pad, c.C)), np.zeros((c.B, c.T + 2 * c.pad, c.C))
    ref[:, c.pad:c.pad + c.T] = val
    if not exact:
        tol[:, c.pad:c.pad + c.T] = 4 * ULP * big + TINY
    return dict(dyp=Ref(ref, tol))


def restate_apply(c, d, defect=None):
    """fp32 in kernel order; defect 'pad_off_by_one': the data rows start one row late"""
    R, C = c.B * c.T, c.C
    ca = d["a"]
    if c.tr:
        invR = f32(1.0) / f32(R)
        mv, iv, db, dg = d["mean"], d["invstd"], d["dbeta"], d["dgamma"]
        c1 = (((-ca * iv).astype(f32) * dg).astype(f32) * invR).astype(f32)
        c0 = ((-ca * (db - ((mv * iv).astype(f32) * dg).astype(f32)).astype(f32)).astype(f32) * invR).astype(f32)
        inner = fma32(c1, d["y"], c0)
    else:
        inner = np.zeros((c.B, c.T, C), f32)
    val = fma32(ca, d["g"], inner)
    out = np.zeros((c.B, c.T + 2 * c.pad, C), f32)
    if defect == "pad_off_by_one":
        n = min(c.T, c.T + c.pad - 1)
        out[:, c.pad + 1:c.pad + 1 + n] = val[:, :n]
    else:
        out[:, c.pad:c.pad + c.T] = val
    return dict(dyp=out)


# ===================================================================================================================== absmax / absmax_multi / fcn_scan
def plan_absmax(n, aligned=True, multi_nmax=None):
    """block count of ign_absmax (cap 2048) or, with multi_nmax, of ign_absmax_multi's grid.x (cap 256, from the largest tensor)"""
    basis = n if multi_nmax is None else multi_nmax
    blocks = min(max(cdiv(basis // 4, 256 * 8), 1), 2048 if multi_nmax is None else 256)
    cls = {"absmax:aligned" if aligned else "absmax:unaligned", "absmax:one_block" if blocks == 1 else "absmax:many_blocks"}
    if aligned:
        cls.add("absmax:scalar_tail" if n % 4 else "absmax:no_tail")
        cls.add("absmax:float4_body" if n >= 4 else "absmax:tail_only")
    return dict(route=f"{blocks} blocks, {'float4 body + tail on block 0' if aligned else 'scalar route'}", blocks=blocks, classes=cls)


ABSMAX_N = (1, 2, 3, 4, 5, 1023, 8193, 16387)
ABSMAX_WHERE = ("first", "last4", "tail", "special")


def absmax_data(n, where, seed):
    """n floats in (-1, 1) with one maximum of magnitude 3 placed, or the `special` mix: -inf's magnitude must win"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, n).astype(f32)
    if where == "first":
        x[0] = -3.0
    elif where == "last4":
        x[max(n // 4 * 4 - 1, 0)] = -3.0               # the last lane of the last float4 (n < 4: element 0)
    elif where == "tail":
        x[n - 1] = 3.0
    elif where == "special":
        x[:] = 0.0
        x[::2] = -0.0
        x[n // 2] = -np.float32(2.0 ** -140)           # a subnormal, negative: the only non-zero magnitude
    elif where == "inf":
        x[n // 3] = -np.inf
    return x


def _absmax_cases():
    rows = [dict(n=n, where=w) for n in ABSMAX_N for w in ABSMAX_WHERE + ("inf",)]
    return [Case("absmax", "exact", **p) for p in rows]


AMM_CASES = [dict(nt=1, sizes=(16387,), off=0), dict(nt=1, sizes=(3,), off=1), dict(nt=2, sizes=(3, 16387), off=0),
             dict(nt=2, sizes=(16387, 3), off=2), dict(nt=16, sizes=(1, 2, 3, 4, 5, 1023, 8193, 16387) * 2, off=5),
             dict(nt=16, sizes=(5,) * 16, off=16)]                     # off: 1-based index of the tensor that starts one float off (0: none)


def _amm_cases():
    return [Case("absmax_multi", "exact", **p) for p in AMM_CASES]


SCAN_CASES = [dict(nl=1, nw=(1,), C=(0,), nzero=0), dict(nl=1, nw=(1025,), C=(0,), nzero=1), dict(nl=1, nw=(1023,), C=(0,), nzero=1025),
              dict(nl=8, nw=(1, 1023, 1025, 1, 1023, 1025, 1, 4097), C=(0, 1, 1024, 1025, 1, 1024, 1025, 7), nzero=8 * 1024 + 1),
              dict(nl=8, nw=(1025,) * 8, C=(0, 1025, 1, 1024, 1025, 1, 1024, 3), nzero=0)]


def _scan_cases():
    return [Case("fcn_scan", r, **p) for p in SCAN_CASES for r in ("gauss", "exact")]


def inputs_scan(c):
    rng, ex = _rng(c), c.regime == "exact"
    d = dict(w=[], gamma=[], beta=[], R=[])
    for l in range(c.nl):
        d["w"].append(_ints(rng, -9, 9, c.nw[l]) if ex else rng.standard_normal(c.nw[l]).astype(f32))
        C = c.C[l]
        d["gamma"].append(None if not C else _ints(rng, -4, 4, C) if ex else rng.standard_normal(C).astype(f32))
        d["beta"].append(None if not C else _ints(rng, -4, 4, C) if ex else rng.standard_normal(C).astype(f32))
        d["R"].append((2, 5, 10, 17, 26, 37, 50, 65)[l] if ex else (2, 3, 800, 12345, 7, 100, 31, 6)[l])       # exact: R - 1 a square
    return d


def reference_scan(c, d):
    """slots (4 nl): 0 = max |w| (exact), 1 = max(|gamma| sqrt(R - 1) + |beta|) within 2 ulp (the square root and the fma round),
    2 and 3 = 0"""
    ref, tol = np.zeros(4 * c.nl), np.zeros(4 * c.nl)
    for l in range(c.nl):
        ref[4 * l] = np.abs(d["w"][l].astype(f64)).max()
        if c.C[l]:
            ref[4 * l + 1] = (np.abs(d["gamma"][l].astype(f64)) * math.sqrt(d["R"][l] - 1) + np.abs(d["beta"][l].astype(f64))).max()
            tol[4 * l + 1] = 0.0 if c.regime == "exact" else 2 * ULP * ref[4 * l + 1]
    return dict(slots=Ref(ref, tol))


# ===================================================================================================================== diversity
DIV_K = (1, 2, 5, 16)
DIV_L = (1, 63, 64, 255, 256, 257, 513)
DIV_REGIMES = ("gauss", "identical", "near", "far")


def plan_div(K, C, L):
    if K > DIV_KMAX:
        return dict(route="IGN_E_UNSUP", refused=IGN_E_UNSUP)
    steps = cdiv(L, 256)
    cls = {f"div:K{K}", f"div:L{L}", f"div:C{C}", "div:one_stride" if steps == 1 else "div:many_strides"}
    if L < 256:
        cls.add("div:idle_threads")
    if L < 64:
        cls.add("div:idle_waves")
    if L % 256 and L > 256:
        cls.add("div:ragged_last_stride")
    if K == 1:
        cls.add("div:no_pairs")
    if K == DIV_KMAX:
        cls.add("div:all_256_pair_threads")
    return dict(route=f"diversity_block x {C}, {steps} strides, {K * (K - 1) // 2} pairs", steps=steps, chain=steps + 6 + 3, classes=cls,
                refused=0)


def _div_cases():
    rows, i = [], 0
    for K in DIV_K:
        for L in DIV_L:
            rows.append(Case("diversity", "gauss", K=K, L=L, C=(1, 3)[i % 2]))
            if K >= 2 and L in (1, 64, 257, 513):
                rows += [Case("diversity", r, K=K, L=L, C=(3, 1)[i % 2]) for r in DIV_REGIMES[1:]]
            i += 1
    return rows


def div_weights(regime, K, C, L, rng):
    """(K, C, L).  identical: shapelet 1 = shapelet 0 (distance exactly eps sqrt(L)); near: shapelet 1 = shapelet 0 + 1e-4 on every
    sample (the two directions of the pair then differ by 4 eps sum(dl) in D^2); far: shapelets about 100 apart -- spread along one
    sample per shapelet, so that every pair is (exp(-100) is subnormal in fp32: the values underflow toward 0)."""
    w = rng.standard_normal((K, C, L)).astype(f32)
    if regime == "identical" and K >= 2:
        w[1] = w[0]
    elif regime == "near" and K >= 2:
        w[1] = (w[0].astype(f64) + 1e-4).astype(f32)
    elif regime == "far":
        w = (0.01 * w).astype(f32)
        w[:, :, 0] += (100.0 * np.arange(K, dtype=f64))[:, None].astype(f32)
    return w


def inputs_div(c):
    return dict(w=div_weights(c.regime, c.K, c.C, c.L, _rng(c)))


def div_f64(w, eps=DIV_EPS):
    """float64: per-channel loss partials (C) and the gradient (K, C, L) of  mean_{c,i,j} exp(-||w_i - w_j + eps||) (1 - delta_ij)"""
    w = np.asarray(w, f64)
    K, C, L = w.shape
    diff = w[:, None] - w[None, :] + eps                                     # (i, j, C, L): w_i - w_j + eps
    D = np.sqrt((diff * diff).sum(-1))                                       # (i, j, C)
    off = ~np.eye(K, dtype=bool)[:, :, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        E = np.where(off, np.exp(-D), 0.0)
        Ew = np.where(off, E / D, 0.0)
    norm = 1.0 / (C * K * K)
    loss_c = E.sum((0, 1)) * norm
    # d e_ij / d w_i = -Ew_ij diff_ij ;  d e_ji / d w_i = +Ew_ji diff_ji   (diff_ji = w_j - w_i + eps)
    # (pair by pair, as the kernel does: a coincident pair's two terms are Ew eps each and cancel, next to terms 1e13 times smaller)
    t = Ew[..., None] * diff
    gw = (t.transpose(1, 0, 2, 3) - t).sum(1) * norm
    return loss_c, gw


def reference_div(c, d):
    loss_c, gw = div_f64(d["w"])
    return dict(loss_part=Ref(loss_c, LOSS_RTOL * np.abs(loss_c) + TINY), gw=Ref(gw, GRAD_RTOL * np.abs(gw).max() + TINY))


def restate_div(w, eps=DIV_EPS, scale=1.0, defect=None):
    """fp32 in kernel order -> (loss partials (C), gw).  defect 'one_d2': D2[j][i] takes the (i, j) sum as well"""
    w = np.asarray(w, f32)
    K, C, L = w.shape
    e32, steps = f32(eps), cdiv(L, 256)
    D2 = np.zeros((K, K, C), f32)

    def blocksum(t):                                  # t (C, L) fp32 addends of the fma chain a = fma(x, x, a)
        full = np.zeros((C, steps * 256), f64)
        full[:, :L] = t
        acc = np.zeros((C, 256), f32)
        for s in range(steps):
            x = full[:, s * 256:(s + 1) * 256]
            acc = (x * x + acc.astype(f64)).astype(f32)
        red = butterfly64(acc.reshape(C, 4, 64))
        return (((red[:, 0] + red[:, 1]).astype(f32) + red[:, 2]).astype(f32) + red[:, 3]).astype(f32)

    for i in range(K):
        for j in range(i + 1, K):
            dl = (w[i] - w[j]).astype(f32)
            D2[i, j] = blocksum((dl + e32).astype(f32))
            D2[j, i] = D2[i, j] if defect == "one_d2" else blocksum((e32 - dl).astype(f32))
    norm = f32(1.0) / (f32(C) * f32(K) * f32(K))
    off = ~np.eye(K, dtype=bool)[:, :, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        D = np.sqrt(D2)
        E = np.where(off, np.exp(-D).astype(f32), f32(0))
        Ew = np.where(off, (E / D).astype(f32), f32(0))
    loss = np.zeros(C, f32)
    for i in range(K):
        for j in range(K):
            loss = (loss + E[i, j]).astype(f32)
    loss = ((loss * norm).astype(f32) * f32(scale)).astype(f32)
    gw = np.zeros((K, C, L), f32)
    for i in range(K):
        g = np.zeros((C, L), f32)
        for j in range(K):
            if j != i:
                dl = (w[i] - w[j]).astype(f32)
                t = ((-Ew[i, j][:, None] * (dl + e32).astype(f32)).astype(f32) + (Ew[j, i][:, None] * (e32 - dl).astype(f32)).astype(f32)).astype(f32)
                g = (g + t).astype(f32)
        gw[i] = ((g * norm).astype(f32) * f32(scale)).astype(f32)
    return loss, gw


# ===================================================================================================================== both regularisers
def plan_reg(G, C, nW):
    if G < 0 or G > REG_GMAX or C <= 0 or nW < 0:
        return dict(route="IGN_E_ARG", refused=IGN_E_ARG, ws_words=0)
    nwb = cdiv(nW, REG_BLOCK)
    nblk = G * C + nwb
    if nblk <= 0:
        return dict(route="IGN_E_ARG", refused=IGN_E_ARG, ws_words=G * C + nwb + 4)
    cls = {f"reg:G{G}", f"reg:nW{nW}", "reg:final_one_stride" if nblk <= 256 else "reg:final_two_strides"}
    if nW % REG_BLOCK:
        cls.add("reg:ragged_last_w_block")
    if nW and nW % 4:
        cls.add("reg:ragged_thread")
    return dict(route=f"sbm_reg_kernel grid {nblk} ({G * C} diversity + {nwb} |W| blocks)", nwb=nwb, nblk=nblk, ws_words=nblk + 4,
                chain=cdiv(nblk, 256) + 8, classes=cls, refused=0)


# K and L differ from group to group
_REG_KL = ((3, 7), (2, 64), (5, 30), (16, 5), (1, 9), (4, 257), (2, 1), (6, 100))
REG_ROWS = [dict(G=1, C=3, nW=0), dict(G=4, C=2, nW=0), dict(G=0, C=1, nW=1), dict(G=0, C=3, nW=3), dict(G=1, C=1, nW=4),
            dict(G=4, C=3, nW=1023), dict(G=8, C=2, nW=1024), dict(G=1, C=5, nW=1025), dict(G=8, C=3, nW=7320), dict(G=0, C=1, nW=7320),
            dict(G=4, C=1, nW=3), dict(G=2, C=122, nW=13 * 1024),                                                  # nblk = 257
            dict(G=4, C=3, nW=1025, lam_reg=0.0), dict(G=4, C=3, nW=1025, lam_div=0.0), dict(G=1, C=2, nW=1025, zeros=1)]


def _reg_cases():
    return [Case("sbm_reg", "gauss", **dict(dict(lam_reg=0.3, lam_div=0.2, zeros=0), **p)) for p in REG_ROWS]


def inputs_reg(c):
    rng = _rng(c)
    W = rng.standard_normal(c.nW).astype(f32)
    if c.zeros:                                      # +0.0 and -0.0 in W: sign(0) = 0 for both
        W[::7], W[3::7] = 0.0, -0.0
    ws = [div_weights("gauss", K, c.C, L, rng) for K, L in _REG_KL[:c.G]]
    return dict(W=W, w=ws)


def reference_reg(c, d):
    """loss = lam_reg mean|W| + lam_div sum_g diversity_g (1e-5 relative); gw_g = lam_div * the float64 diversity gradient (1e-4 of
    its maximum); gW_reg = lam_reg sign(W) / nW: the quotient rounds once -> 1 ulp, and 0 where W is +-0"""
    lr, ld = float(f32(c.lam_reg)), float(f32(c.lam_div))
    loss = lr * np.abs(d["W"].astype(f64)).mean() if c.nW else 0.0
    out = {}
    for g, w in enumerate(d["w"]):
        lc, gw = div_f64(w)
        loss += ld * lc.sum()
        out[f"gw{g}"] = Ref(ld * gw, GRAD_RTOL * np.abs(ld * gw).max() + TINY)
    out["loss"] = Ref(np.array([loss]), LOSS_RTOL * abs(loss) + TINY)
    if c.nW:
        gref = lr * np.sign(d["W"].astype(f64)) / c.nW
        out["gW_reg"] = Ref(gref, ULP * np.abs(gref))
    return out


def restate_reg(c, d):
    """fp32 in kernel order -> the loss"""
    lr, ld, G, C = f32(c.lam_reg), f32(c.lam_div), c.G, c.C
    pl = plan_reg(G, C, c.nW)
    parts = np.zeros(pl["nblk"], f32)
    for g, w in enumerate(d["w"]):
        parts[g * C:(g + 1) * C] = restate_div(w, scale=ld)[0]
    if c.nW:
        sc = lr / f32(c.nW)
        full = np.zeros(pl["nwb"] * REG_BLOCK, f32)
        full[:c.nW] = np.abs(d["W"])
        a = seqsum32(full.reshape(pl["nwb"], 256, 4), 2)
        parts[G * C:] = (seqsum32(a, 1) * sc).astype(f32)
    return reg_final_sum(parts)


def reg_final_sum(parts):
    n = len(parts)
    full = np.zeros(cdiv(n, 256) * 256, f32)
    full[:n] = parts
    red = seqsum32(full.reshape(-1, 256), 0)
    o = 128
    while o:
        red[:o] = (red[:o] + red[o:2 * o]).astype(f32)
        o //= 2
    return red[0]


class RegWorkspace:
    """What sbm_reg_kernel does to its workspace, word for word.  ticket_at='fixed': the ticket is word REG_TICKET_WORD and the
    partials start at REG_PARTS_WORD; 'after_parts': the ticket follows the nblk partials, which start at word 0 (the defect)."""

    def __init__(self, words, ticket_at="fixed"):
        self.w, self.ticket_at = np.zeros(words, np.uint32), ticket_at

    def call(self, parts):
        """-> the loss written, or None when no block draws the last ticket"""
        parts = np.asarray(parts, f32)
        nblk = len(parts)
        tk, p0 = (REG_TICKET_WORD, REG_PARTS_WORD) if self.ticket_at == "fixed" else (nblk, 0)
        loss = None
        for blk in range(nblk):
            self.w[p0 + blk] = parts[blk:blk + 1].view(np.uint32)[0]
            old = int(self.w[tk])
            self.w[tk] = (old + 1) & 0xFFFFFFFF
            if old == nblk - 1:
                loss = reg_final_sum(self.w[p0:p0 + nblk].view(f32))
                self.w[tk] = 0
        return loss


# sequence (b): large nblk, then small, then large, on one buffer sized for the large one
REG_SEQ_B = (dict(G=8, C=3, nW=7320), dict(G=1, C=3, nW=1), dict(G=8, C=3, nW=7320))
REG_SEQ_A = dict(G=4, C=3, nW=1025)


# ===================================================================================================================== refusals (checked before any launch)
# (entry point, what is wrong, the return code) -- tests/test_gpu_glue_edges.py builds each call
REFUSALS = [
    ("head_fwd", "F%4", IGN_E_ARG), ("head_fwd", "ldx%4", IGN_E_ARG), ("head_fwd", "ldx<F", IGN_E_ARG), ("head_fwd", "W_misaligned", IGN_E_ARG),
    ("head_fwd", "X_misaligned", IGN_E_ARG), ("head_fwd", "N257", IGN_E_UNSUP),
    ("head_bwd", "F%4", IGN_E_ARG), ("head_bwd", "ldx%4", IGN_E_ARG), ("head_bwd", "ldx<F", IGN_E_ARG), ("head_bwd", "W_misaligned", IGN_E_ARG),
    ("head_bwd", "N257", IGN_E_UNSUP), ("head_bwd", "B641_N16", IGN_E_TOOBIG), ("head_bwd", "B3414_N3", IGN_E_TOOBIG),
    ("diversity", "K17", IGN_E_UNSUP), ("sbm_reg", "K17", IGN_E_UNSUP), ("sbm_reg", "G9", IGN_E_ARG), ("sbm_reg", "nothing", IGN_E_ARG),
    ("bn_relu_pool_fwd", "C6", IGN_E_ARG), ("bn_relu_pool_fwd", "C1028", IGN_E_ARG), ("bn_relu_pool_head_fwd", "C6", IGN_E_ARG),
    ("bn_relu_pool_head_fwd", "C1028", IGN_E_ARG), ("bn_relu_pool_bwd", "C6", IGN_E_ARG), ("bn_relu_pool_bwd", "C1028", IGN_E_ARG),
    ("bn_bwd_apply", "C6", IGN_E_ARG), ("bn_bwd_apply", "C1028", IGN_E_ARG), ("absmax_multi", "n17", IGN_E_ARG), ("absmax", "misaligned", IGN_E_ARG),
    ("fcn_scan", "nl9", IGN_E_ARG),
]


# ===================================================================================================================== the table
@functools.lru_cache(maxsize=None)
def cases():
    affine = [Case("bn_affine_eval", r, C=C) for C in AFFINE_C for r in ("gauss", "exact")]
    return tuple(_head_fwd_cases() + _head_bwd_cases() + _finalize_cases() + affine + _pool_fwd_cases() + _pool_bwd_cases() + _apply_cases()
                 + _absmax_cases() + _amm_cases() + _scan_cases() + _div_cases() + _reg_cases())


def of(entry):
    return [c for c in cases() if c.entry == entry]


def plan(c):
    e = c.entry
    if e == "head_fwd":
        return plan_head_fwd(c.F, c.N, c.B, c.F + c.pad, c.bias)
    if e == "head_bwd":
        return plan_head_bwd(c.B, c.F, c.N, c.mode, c.gbias, c.add)
    if e in ("bn_finalize_fwd", "bn_finalize_bwd"):
        pl = plan_bn_sum(c.nparts, c.C)
        pl["classes"] = pl["classes"] | {"fin:R1" if c.nparts * c.rpp == 1 else "fin:R>1", "fin:running" if c.run else "fin:no_running"}
        return pl
    if e == "bn_affine_eval":
        return dict(route=f"grid {cdiv(c.C, 256)}", chain=0, classes={f"affine:C{c.C}"})
    if e == "bn_relu_pool_fwd":
        pl = plan_pool(c.C, c.T)
        pl["classes"] = pl["classes"] | ({f"pool:head_N{c.N}", "pool:head_bias" if c.bias else "pool:head_nobias"} if c.N else {"pool:headless"})
        return pl
    if e == "bn_relu_pool_bwd":
        pl = plan_pool_bwd(c.C, c.T, c.B)
        pl["classes"] = pl["classes"] | {"poolbwd:part" if c.part else "poolbwd:nopart"}
        return pl
    if e == "bn_bwd_apply":
        pl = plan_apply(c.B, c.T, c.C, c.pad)
        pl["classes"] = pl["classes"] | {f"apply:slot_{c.slot}", "apply:training" if c.tr else "apply:eval"}
        if c.slot != "none" and 256 % (c.C // 4):
            pl["classes"].add("apply:slot_with_dead_lanes")
        pl["chain"] = 0
        return pl
    if e == "absmax":
        pl = plan_absmax(c.n)
        pl["classes"] = pl["classes"] | {f"absmax:max_{c.where}", f"absmax:n{c.n}"}
        pl["chain"] = 0
        return pl
    if e == "absmax_multi":
        cls = {f"amm:{c.nt}_tensors"} | ({"amm:unaligned_tensor"} if c.off else set())
        if 3 in c.sizes and 16387 in c.sizes:
            cls.add("amm:sizes_3_and_16387")
        return dict(route=f"grid ({plan_absmax(0, multi_nmax=max(c.sizes))['blocks']}, {c.nt})", chain=0, classes=cls)
    if e == "fcn_scan":
        cls = {f"scan:nl{c.nl}", f"scan:nzero{'0' if c.nzero == 0 else '1' if c.nzero == 1 else '>grid'}"}
        cls |= {f"scan:nw{n}" for n in c.nw} | {f"scan:C{C}" for C in c.C}
        return dict(route=f"grid {c.nl} x 1024", chain=0, classes=cls)
    if e == "diversity":
        pl = plan_div(c.K, c.C, c.L)
        pl["classes"] = pl["classes"] | {f"div:{c.regime}"}
        return pl
    if e == "sbm_reg":
        pl = plan_reg(c.G, c.C, c.nW)
        if c.lam_reg == 0:
            pl["classes"].add("reg:lam_reg0")
        if c.lam_div == 0:
            pl["classes"].add("reg:lam_div0")
        if c.zeros:
            pl["classes"].add("reg:signed_zeros")
        if c.nW == 0 and c.G:
            pl["classes"].add("reg:no_W")
        return pl
    raise KeyError(e)


@functools.lru_cache(maxsize=64)
def inputs(c):
    return {"head_fwd": inputs_head_fwd, "head_bwd": inputs_head_bwd, "bn_finalize_fwd": inputs_finalize, "bn_finalize_bwd": inputs_finalize,
            "bn_affine_eval": inputs_affine, "bn_relu_pool_fwd": inputs_pool_fwd, "bn_relu_pool_bwd": inputs_pool_bwd, "bn_bwd_apply": inputs_apply,
            "fcn_scan": inputs_scan, "diversity": inputs_div, "sbm_reg": inputs_reg}[c.entry](c)


def reference(c):
    d = inputs(c)
    return {"head_fwd": reference_head_fwd, "head_bwd": reference_head_bwd, "bn_finalize_fwd": reference_finalize,
            "bn_finalize_bwd": reference_finalize, "bn_affine_eval": reference_affine, "bn_relu_pool_fwd": reference_pool_fwd,
            "bn_relu_pool_bwd": reference_pool_bwd, "bn_bwd_apply": reference_apply, "fcn_scan": reference_scan, "diversity": reference_div,
            "sbm_reg": reference_reg}[c.entry](c, d)


# every branch class the table has to reach (tests/test_glue_edges_host.py proves it does)
REQUIRED_CLASSES = (
    ["fwd:nthr256", "fwd:nthr1024", "fwd:bias", "fwd:nobias", "fwd:ldx=F", "fwd:ldx>F", "fwd:one_step", "fwd:many_steps", "fwd:idle_threads",
     "fwd:ragged_last_step", "fwd:idle_waves", "fwd:N17"] + [f"fwd:N{n}" for n in HEAD_FWD_N] + [f"fwd:F{f}" for f in HEAD_FWD_F] + ["fwd:B1", "fwd:B3"]
    + [f"bwd:{m}:{g}" for m in ("xw", "x", "w") for g in ("gbias", "nogbias")] + ["bwd:add_none", "bwd:add_scaled", "bwd:add_unscaled"]
    + [f"bwd:B{b}" for b in HEAD_BWD_B] + [f"bwd:F{f}" for f in HEAD_BWD_F]
    + ["bwd:per1", "bwd:per>1", "bwd:empty_group_b0>B", "bwd:empty_group_b0=B", "bwd:short_last_group", "bwd:ragged_f_slice", "bwd:one_short_slice",
       "bwd:two_x_blocks", "bwd:ragged_x_block", "bwd:lds_at_limit"]
    + [f"fin:C{c}" for c in FIN_C] + [f"fin:nparts{n}" for n in FIN_NPARTS] + ["fin:per1", "fin:per>1", "fin:empty_slices", "fin:short_last_slice", "fin:flush_at_slice_end",
                                     "fin:flush_one_before_slice_end", "fin:flush_inside_slice", "fin:ragged_channel_block", "fin:many_channel_blocks",
                                     "fin:one_short_channel_block", "fin:R1", "fin:R>1", "fin:running", "fin:no_running"]
    + [f"affine:C{c}" for c in AFFINE_C]
    + [f"pool:C{c}" for c in POOL_C] + [f"pool:rif{r}" for r in POOL_RIF]
    + ["pool:idle_threads", "pool:no_idle_threads", "pool:T<rif", "pool:T=rif", "pool:T=rif-1", "pool:T=k*rif+1", "pool:several_columns_per_thread",
       "pool:headless", "pool:head_bias", "pool:head_nobias"] + [f"pool:head_N{n}" for n in POOL_HEAD_N]
    + [f"poolbwd:T{t}" for t in POOL_BWD_T] + ["poolbwd:one_block", "poolbwd:many_blocks", "poolbwd:short_last_block", "poolbwd:one_row_last_block",
                                              "poolbwd:part", "poolbwd:nopart"]
    + [f"apply:pad{p}" for p in APPLY_PADS] + [f"apply:rows{r}" for r in APPLY_ROWSETS]
    + ["apply:one_block", "apply:many_blocks", "apply:short_last_block", "apply:dead_lanes_in_last_wave", "apply:slot_none", "apply:slot_zero",
       "apply:slot_above", "apply:slot_with_dead_lanes", "apply:training", "apply:eval", "apply:C12", "apply:C24", "apply:C260"]
    + [f"absmax:n{n}" for n in ABSMAX_N] + [f"absmax:max_{w}" for w in ABSMAX_WHERE + ("inf",)]
    + ["absmax:aligned", "absmax:one_block", "absmax:many_blocks", "absmax:scalar_tail", "absmax:no_tail", "absmax:float4_body", "absmax:tail_only"]
    + ["amm:1_tensors", "amm:16_tensors", "amm:unaligned_tensor", "amm:sizes_3_and_16387"]
    + ["scan:nl1", "scan:nl8", "scan:nw1", "scan:nw1023", "scan:nw1025", "scan:C0", "scan:C1", "scan:C1024", "scan:C1025", "scan:nzero0", "scan:nzero1",
       "scan:nzero>grid"]
    + [f"div:K{k}" for k in DIV_K] + [f"div:L{l}" for l in DIV_L] + ["div:C1", "div:C3"] + [f"div:{r}" for r in DIV_REGIMES]
    + ["div:one_stride", "div:many_strides", "div:idle_threads", "div:idle_waves", "div:ragged_last_stride", "div:no_pairs", "div:all_256_pair_threads"]
    + [f"reg:G{g}" for g in (0, 1, 4, 8)] + [f"reg:nW{n}" for n in (0, 1, 3, 4, 1023, 1024, 1025, 7320)]
    + ["reg:final_one_stride", "reg:final_two_strides", "reg:ragged_last_w_block", "reg:ragged_thread", "reg:lam_reg0", "reg:lam_div0",
       "reg:signed_zeros", "reg:no_W"])
