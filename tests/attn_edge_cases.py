"""The case tables of the attention edge tests and the tile geometry they rest on (tests/test_attn_edges_host.py proves that every
(arithmetic, head width) route meets every tail class and that the regime inputs are what they claim; tests/test_gpu_attn_edges.py
runs the rows against float64 on an MI355X; tests/diag_attn_edges.py records both in profiles/attn_edges.json).  torch is imported
inside the functions only.

The kernels: csrc/ign_attention.hip (fp32 MFMA), csrc/ign_attention_x6.hip (the split arithmetics: three bf16 planes "bf16x6", two
fp16 planes "f16x3", one bf16 plane "bf16" inside autocast), csrc/ign_attention_map.hip (the map of need_weights=True)."""
import functools
import math

# ------------------------------------------------------------------------------------------------ the kernels' geometry
ATTN_MATH_F32, ATTN_MATH_X6, ATTN_MATH_BF16, ATTN_MATH_H3 = 0, 1, 2, 3      # ops.ATTN_MATH_* / include/ign_abi.h
WG_QUERIES = 128                  # queries per workgroup: forward, dQ and map kernels of every family (blockIdx.x * 128)
WAVE_QUERIES = 32                 # queries (or keys, in dK / dV) per wave: one per lane & 31
SUB_KEYS = 32                     # keys per score tile (one 32x32 MFMA accumulator) in every kernel
ATT_KT = 64                       # csrc/ign_attention.hip: rows staged per LDS tile, forward and both backward kernels
MAP_KT = 64                       # csrc/ign_attention_map.hip: keys staged per LDS tile
AB_T = 32                         # csrc/ign_attention_x6.hip: rows per staged tile of the split backward kernels
DKV_WG_KEYS = 128                 # keys per dK / dV workgroup, both families
HEAD_WIDTHS = (16, 32, 64, 128)


def x6_key_tile(E):
    """AxPitch<E>::KT: keys staged per LDS tile of attn_fwd_x6_kernel"""
    return 64 if E == 16 else 32


# ------------------------------------------------------------------------------------------------ bounds (none of them new)
FWD_TOL, GRAD_TOL = 2e-5, 5e-5                      # tests/test_gpu_baselines.py::test_attention_vs_fp64_reference
MAP_ROWSUM_TOL = 1e-5                               # tests/test_gpu_attn_map.py::test_map_vs_fp64_and_consistent_with_the_output
MAP_TOL = {"bf16": 1e-4}                            # ... map vs float64, else FWD_TOL
MAP_OUT_TOL = {"bf16": 3e-2}                        # ... float64 attn @ v vs out, else FWD_TOL
BF16_DROPOUT_FWD_TOL, BF16_DROPOUT_GRAD_TOL = 3e-2, 5e-2    # tests/test_gpu_attn_dropout.py, the autocast test (unrounded float64)
REGIME_MARGIN = 8                                   # tolerance = max(project bound, 8 x the fp32 restatement's error)
REGIME_MAX_FACTOR = 4                               # ... and never more than 4 x the project bound (else the row is rescaled)
SCORE_RANGE = (12.0, 24.0)                          # max |scale q . k| of every regime but "zero"

# ------------------------------------------------------------------------------------------------ routes
# (arithmetic, E).  At E = 128 the split arithmetics have a split forward only (the split backward spills and is not routed to):
# "f16x3" and "bf16x6" resolve to the same kernels there, kept once.  A call that is differentiated runs forward and backward on the
# fp32-MFMA kernels (one family: see ops._attn_arith), a call that is not runs the split forward.
ROUTES = ([("f32", E) for E in HEAD_WIDTHS] + [("bf16x6", E) for E in HEAD_WIDTHS] + [("f16x3", E) for E in (16, 32, 64)]
          + [("bf16", E) for E in (16, 32, 64)])


def knobs(amath):
    """(ops.ATTN_MATH, ops.GEMM_MATH, autocast) that select the arithmetic"""
    if amath == "bf16":
        return "bf16x6", "f16x3", True
    return ("bf16x6" if amath == "f16x3" else amath), ("f16x3" if amath == "f16x3" else "bf16x6"), False


def route_arith(amath, E):
    """(forward, backward) ATTN_MATH_* of a differentiated call on the route"""
    if amath == "f32" or E > 64:
        return ATTN_MATH_F32, ATTN_MATH_F32
    if amath == "bf16":
        return ATTN_MATH_BF16, ATTN_MATH_BF16
    return (ATTN_MATH_H3, ATTN_MATH_H3) if amath == "f16x3" else (ATTN_MATH_X6, ATTN_MATH_X6)


def inference_arith(amath, E):
    """ATTN_MATH_* of the forward of a call that is not differentiated"""
    return ATTN_MATH_X6 if (amath != "f32" and E > 64) else route_arith(amath, E)[0]


def fwd_key_tile(fwd_arith, E):
    return ATT_KT if fwd_arith == ATTN_MATH_F32 else x6_key_tile(E)


def bwd_row_tile(bwd_arith):
    return ATT_KT if bwd_arith == ATTN_MATH_F32 else AB_T


def batch_heads(E):
    """(B, H) of the table rows: both offsets exercised, H odd; one batch of two heads at E = 128"""
    return (1, 2) if E == 128 else (2, 3)


# ------------------------------------------------------------------------------------------------ the edge table
EDGE_PAIRS = [(1, 1), (1, 129), (129, 1), (31, 33), (33, 31), (32, 32), (64, 64), (63, 65), (65, 63), (96, 97), (97, 96),
              (128, 128), (127, 129), (129, 127), (161, 95), (5, 161)]
DROPOUT_PAIRS = [(33, 31), (129, 127), (5, 161)]
PACKED_LENGTHS = (33, 129)
UNROUTED_PAIRS = [(33, 31), (129, 127), (5, 161)]   # ign_attn_bwd_x6 / _strided at E = 128

# classes of the query count: below / at / above one wave, below / at / above one workgroup, a second workgroup with a full wave
L_CLASSES = {
    "1": lambda L: L == 1,
    "wave - 1": lambda L: L == WAVE_QUERIES - 1,
    "wave": lambda L: L == WAVE_QUERIES,
    "wave + 1": lambda L: L == WAVE_QUERIES + 1,
    "workgroup - 1": lambda L: L == WG_QUERIES - 1,
    "workgroup": lambda L: L == WG_QUERIES,
    "workgroup + 1": lambda L: L == WG_QUERIES + 1,
    "above workgroup + wave": lambda L: L > WG_QUERIES + WAVE_QUERIES,
}
# classes of the key count, the same for every route: the sizes around one and two score tiles, one and two 64-key LDS tiles
S_CLASSES = {
    "1": lambda S: S == 1,
    "below one score tile": lambda S: 1 < S < SUB_KEYS,
    "32": lambda S: S == SUB_KEYS,
    "33": lambda S: S == SUB_KEYS + 1,
    "63": lambda S: S == 2 * SUB_KEYS - 1,
    "64": lambda S: S == 2 * SUB_KEYS,
    "65": lambda S: S == 2 * SUB_KEYS + 1,
    "96": lambda S: S == 3 * SUB_KEYS,
    "97": lambda S: S == 3 * SUB_KEYS + 1,
    "127": lambda S: S == DKV_WG_KEYS - 1,
    "128": lambda S: S == DKV_WG_KEYS,
    "129": lambda S: S == DKV_WG_KEYS + 1,
}


def branch_classes(amath, E):
    """the tail branches of the kernels a route runs, as predicates of (L, S), from the geometry above"""
    fwd, bwd = route_arith(amath, E)
    BT = bwd_row_tile(bwd)
    c = {
        "forward: last score tile full (no key masked)": lambda L, S: S % SUB_KEYS == 0,
        "forward: last score tile ragged": lambda L, S: S % SUB_KEYS != 0,
        "a second query workgroup with one live query": lambda L, S: L % WG_QUERIES == 1 and L > WG_QUERIES,
        "a second dK / dV workgroup with one live key": lambda L, S: S % DKV_WG_KEYS == 1 and S > DKV_WG_KEYS,
        "fewer queries than one wave": lambda L, S: L < WAVE_QUERIES,
        "backward: last staged query tile ragged": lambda L, S: L % BT != 0,
        "backward: last staged query tile full": lambda L, S: L % BT == 0,
        "backward: more than one staged query tile": lambda L, S: L > BT,
        "map: second score tile of the LDS tile skipped": lambda L, S: 1 <= S % MAP_KT <= SUB_KEYS,
    }
    for KT in {fwd_key_tile(fwd, E), fwd_key_tile(inference_arith(amath, E), E)}:      # both forwards of the route
        c[f"forward, {KT}-key LDS tiles: more than one"] = lambda L, S, KT=KT: S > KT
        c[f"forward, {KT}-key LDS tiles: exactly one, full"] = lambda L, S, KT=KT: S == KT
        if KT == 2 * SUB_KEYS:
            c[f"forward, {KT}-key LDS tiles: second score tile skipped"] = lambda L, S, KT=KT: 1 <= S % KT <= SUB_KEYS
            c[f"forward, {KT}-key LDS tiles: second score tile ragged"] = lambda L, S, KT=KT: S % KT > SUB_KEYS
    return c


# ------------------------------------------------------------------------------------------------ metric
def slice_err(got, ref, floor=0.0, dims=(1, 3)):
    """max over the (batch, head) slices of max |got - ref| / max |ref|, both maxima over `dims` of the slice ((B, N, H, E): (1, 3);
    the (B, H, L, S) map: (2, 3)).  `floor` is the least denominator: where the true value is identically zero (the reference holds
    zeros or its own rounding noise) the error is judged against it; with floor 0 a zero reference must be met exactly."""
    import torch
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not torch.isfinite(got).all():
        return math.inf
    diff, den = (got - ref).abs().amax(dims), ref.abs().amax(dims)
    den = den.clamp_min(float(floor))
    err = torch.where(diff == 0, torch.zeros_like(diff), diff / den)      # x / 0 = inf for x > 0
    return float(err.max())


def whole_err(got, ref):
    """max |got - ref| / max |ref| over the whole tensor: the metric of the tests whose bounds the bf16 route is held to"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12))


def zero_floors(q, k, v, go, scale, S):
    """{tensor: floor} for the gradients that are identically zero: with one key the softmax is constant, dq = dk = 0, and what
    the kernels leave there is judged against the natural scale of the products it cancels from"""
    if S != 1:
        return {}
    E = q.shape[-1]
    nat = abs(scale) * E * float(go.abs().max()) * float(v.abs().max())
    return {"dq": nat * float(k.abs().max()), "dk": nat * float(q.abs().max())}


# ------------------------------------------------------------------------------------------------ inputs and references
def scale_of(E):
    return 1.0 / math.sqrt(E)


@functools.lru_cache(maxsize=None)
def edge_inputs(L, S, E):
    """(q, k, v, dO) fp32 on the CPU, the same for every route; callers must not modify them"""
    import torch
    B, H = batch_heads(E)
    g = torch.Generator().manual_seed(100003 * L + 1009 * S + E)
    return tuple(torch.randn(B, n, H, E, generator=g) for n in (L, S, S, L))


def float64_attention(q, k, v, go, scale):
    """softmax(scale Q K^T) V, its gradients under dO, and the (B, H, L, S) map, in float64 on the CPU (the formula of
    tests/test_gpu_baselines.py::_attn_ref)"""
    import torch
    qr, kr, vr = (t.detach().double().cpu().requires_grad_(True) for t in (q, k, v))
    p = torch.softmax(scale * torch.einsum("blhe,bshe->bhls", qr, kr), dim=-1)
    o = torch.einsum("bhls,bshd->blhd", p, vr)
    (o * go.detach().double().cpu()).sum().backward()
    return dict(out=o.detach(), dq=qr.grad, dk=kr.grad, dv=vr.grad, probs=p.detach())


def fp32_restatement(q, k, v, go, scale):
    """the same formula evaluated in float32 by torch on the CPU (scores, softmax, both products, autograd)"""
    import torch
    qr, kr, vr = (t.detach().float().cpu().requires_grad_(True) for t in (q, k, v))
    p = torch.softmax(scale * torch.einsum("blhe,bshe->bhls", qr, kr), dim=-1)
    o = torch.einsum("bhls,bshd->blhd", p, vr)
    (o * go.detach().float().cpu()).sum().backward()
    return dict(out=o.detach(), dq=qr.grad, dk=kr.grad, dv=vr.grad)


@functools.lru_cache(maxsize=None)
def edge_reference(L, S, E):
    return float64_attention(*edge_inputs(L, S, E), scale_of(E))


# ------------------------------------------------------------------------------------------------ score regimes
REGIME_SHAPE = (2, 70, 161, 2)                      # B, L, S, H: 161 keys leave a ragged last tile at both key-tile sizes
REGIME_WIDTHS = (16, 64, 128)
REGIMES = ("sharp", "rising", "falling", "last", "tie", "uniform", "zero")
REGIME_TARGET = 18.0                                # max |scale q . k| the inputs are normalised to
TIE_KEYS = (5, REGIME_SHAPE[2] - 1)                 # the two keys that share the maximum: first tile and the ragged last one
TIE_ROWS = (0, 33, 69)                              # the queries that tie (one per wave that has a live query, first and last row)
TIE_V, TIE_DO = 2.0, 0.5                            # |v| and |dO| of the tie regime: constant magnitude, random sign
TIE_OTHER_ROWS_TARGET = 4.0                         # max |score| of the tie regime's ordinary rows


def regime_routes():
    """(regime, arithmetic, E) of every regime case: every route at the widths of REGIME_WIDTHS"""
    return [(r, a, E) for r in REGIMES for a, E in ROUTES if E in REGIME_WIDTHS]


def _max_score(q, k, scale):
    import torch
    return float((scale * torch.einsum("blhe,bshe->bhls", q.double(), k.double())).abs().max())


# The bf16 route's rows of the regimes whose dq cancels over nearly collinear keys, rescaled until its tolerances obey their
# condition (bf16_regime_tolerances).  rising / falling: q_i = a_i u exactly and every key gets a component of `key_noise` x |u|
# orthogonal to u in a direction of its own -- the scores stay the ramp, dq = scale sum_j dS_j k_j no longer cancels -- at a lower
# maximum score.  last: a lower maximum score and a smaller common offset of the other keys.
BF16_RESCALED = dict(rising=dict(target=13.0, key_noise=1.0), falling=dict(target=13.0, key_noise=1.0), last=dict(target=14.0, offset=0.4))


@functools.lru_cache(maxsize=None)
def regime_inputs(name, E, bf16=False):
    """(q, k, v, dO) fp32 on the CPU; callers must not modify them.  bf16: the rows the bf16 route runs (BF16_RESCALED).
    sharp: random q, k, q scaled up.  rising: k_j = (j / (S - 1)) u + noise, q_i = a_i u + noise with a_i > 0: the scores of every
    row grow with the key index, so its running maximum moves in every tile.  falling: the same with the keys reversed: the
    maximum is in the first tile.  last: one dominant key at S - 1.  tie: the rows TIE_ROWS score exactly the same on the two keys
    TIE_KEYS (which differ only where those q are zero) and far less elsewhere; v is +-TIE_V with v[j2] = -v[j1], dO is +-TIE_DO
    and, on the tie rows, the sign pattern of v[j1]: p = 1/2 on both keys, dP = +-E TIE_V TIE_DO, delta = 0, |dS| = E TIE_V TIE_DO
    / 2, a quarter of the f16x3 kernels' hard bound 2 E max|dO| max|v|.  uniform: all keys identical.  zero: q = 0."""
    import torch
    B, L, S, H = REGIME_SHAPE
    scale = scale_of(E)
    g = torch.Generator().manual_seed(7919 * REGIMES.index(name) + E)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    q, k, v, go = rn(B, L, H, E), rn(B, S, H, E), rn(B, S, H, E), rn(B, L, H, E)
    u = rn(B, 1, H, E)
    a = 0.75 + 0.5 * torch.rand(B, L, H, 1, generator=g, dtype=torch.float64)
    unit = lambda t: t / t.norm(dim=-1, keepdim=True) * E ** 0.25          # scale * t . t = 1
    re = BF16_RESCALED.get(name) if bf16 else None
    target = re["target"] if re else REGIME_TARGET
    if name in ("rising", "falling"):
        ramp = torch.linspace(0.0, 1.0, S, dtype=torch.float64).view(1, S, 1, 1)
        ramp = ramp if name == "rising" else ramp.flip(1)
        if re:
            uh = u / u.norm(dim=-1, keepdim=True)
            w = k - (k * uh).sum(-1, keepdim=True) * uh
            k = ramp * unit(u) + re["key_noise"] * unit(w)
            q = a * unit(u)
        else:
            k = ramp * unit(u) + 0.003 * k
            q = a * unit(u) + 0.3 * q
    elif name == "last":
        k = (re["offset"] if re else 0.5) * unit(u) + 0.2 * k            # a common offset: the other keys keep some weight
        k[:, S - 1] = unit(u)[:, 0]
        q = (0.9 + 0.4 * (a - 0.75)) * unit(u) + 0.1 * q
    elif name == "tie":
        half = E // 2
        u[..., half:] = 0
        ut = unit(u)
        w = torch.zeros(B, 1, H, E, dtype=torch.float64)
        w[..., half:] = rn(B, 1, H, E - half)
        j1, j2 = TIE_KEYS
        k = 0.3 * k
        k[:, j1], k[:, j2] = (ut + w)[:, 0], (ut - w)[:, 0]
        rows = list(TIE_ROWS)
        q[:, rows] = 0
        q = q * (TIE_OTHER_ROWS_TARGET / _max_score(q, k, scale))
        for n, i in enumerate(rows):
            q[:, i] = (1.0 - 0.1 * n) * REGIME_TARGET * ut[:, 0]
        v = TIE_V * torch.sign(v)
        v[:, j2] = -v[:, j1]
        go = TIE_DO * torch.sign(go)
        go[:, rows] = TIE_DO * torch.sign(v[:, j1])[:, None]
    elif name == "uniform":
        k = k[:, :1].expand(B, S, H, E).contiguous()
    elif name == "zero":
        q = torch.zeros_like(q)
    if name not in ("zero", "tie"):
        q = q * (target / _max_score(q, k, scale))
    return tuple(t.float().contiguous() for t in (q, k, v, go))


@functools.lru_cache(maxsize=None)
def regime_reference(name, E):
    return float64_attention(*regime_inputs(name, E), scale_of(E))


def bf16_model_err(got, model, floor=None):
    """(max, rms) distance to the rounded-operand model, each over the model's own max / rms (the metrics of
    tests/test_gpu_bf16_parity.py); `floor`: the least denominator, for a gradient that is identically zero before rounding"""
    import torch
    got, model = got.detach().double().cpu(), model.detach().double().cpu()
    d = got - model
    if not torch.isfinite(d).all():
        return math.inf, math.inf
    res = []
    for num, den in ((float(d.abs().max()), float(model.abs().max())), (float(d.square().mean().sqrt()), float(model.square().mean().sqrt()))):
        den = max(den, 1e-12) if floor is None else max(den, floor)
        res.append(0.0 if num == 0 else (num / den if den > 0 else math.inf))
    return tuple(res)


BF16_NOISE_SEEDS = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def regime_bf16_model(name, E):
    from test_gpu_bf16_parity import _attn_model
    return _attn_model(*regime_inputs(name, E, True), scale_of(E))


def _bf16_tolerances(inputs, scale, clean, floors):
    from test_gpu_bf16_parity import ATTN_FACTOR, ATTN_TOL, ATTN_TOL_RMS, _attn_model, _fp32_noise
    noise = {what: [0.0, 0.0] for what in ("out", "dq", "dk", "dv")}
    for seed in BF16_NOISE_SEEDS:
        noisy = _attn_model(*inputs, scale, pre=_fp32_noise(seed))
        for what in noise:
            noise[what] = [max(a, b) for a, b in zip(noise[what], bf16_model_err(noisy[what], clean[what], floors.get(what)))]
    return {what: ((max(ATTN_TOL, ATTN_FACTOR * n[0]), max(ATTN_TOL_RMS, ATTN_FACTOR * n[1])), tuple(n)) for what, n in noise.items()}


@functools.lru_cache(maxsize=None)
def bf16_regime_tolerances(name, E):
    """{tensor: ((max tolerance, rms tolerance), (max noise, rms noise))} of the bf16 route.  The bounds of
    tests/test_gpu_bf16_parity.py are ATTN_FACTOR x the model's own fp32 noise floor (the model run again with every fp32
    intermediate in front of a rounding point moved by 2^-23) on that file's random shapes; a regime row that cancels over its keys
    shows one flipped rounding amplified, so the same measurement is taken on the case itself, over BF16_NOISE_SEEDS:
    max(that file's bound, ATTN_FACTOR x noise).  As for the fp32-accurate routes no tolerance may exceed REGIME_MAX_FACTOR x
    that file's bound (tests/test_attn_edges_host.py); the rows that did are rescaled (BF16_RESCALED)."""
    return _bf16_tolerances(regime_inputs(name, E, True), scale_of(E), regime_bf16_model(name, E), regime_zero_floors(name, E))


@functools.lru_cache(maxsize=None)
def edge_bf16_model(L, S, E):
    from test_gpu_bf16_parity import _attn_model
    return _attn_model(*edge_inputs(L, S, E), scale_of(E))


def regime_zero_floors(name, E):
    """q = 0 makes dk = scale dS^T q identically zero: floor scale E max|dO| max|v| max|q| = 0, the kernels must return zeros.
    Identical keys k_j = k_0 make dq = scale k_0 sum_j dS_ij identically zero too (the rows of dS sum to zero): the float64
    reference holds its own rounding noise there, and the floor is the natural scale scale E max|dO| max|v| max|k|."""
    if name == "zero":
        return {"dk": 0.0}
    if name == "uniform":
        q, k, v, go = regime_inputs(name, E)
        return {"dq": scale_of(E) * E * float(go.abs().max()) * float(v.abs().max()) * float(k.abs().max())}
    return {}


@functools.lru_cache(maxsize=None)
def regime_tolerances(name, E):
    """{tensor: (tolerance, fp32 restatement's error, project bound)} in the slice metric"""
    ref = regime_reference(name, E)
    r32 = fp32_restatement(*regime_inputs(name, E), scale_of(E))
    floors = regime_zero_floors(name, E)
    out = {}
    for what in ("out", "dq", "dk", "dv"):
        bound = FWD_TOL if what == "out" else GRAD_TOL
        e32 = slice_err(r32[what], ref[what], floor=floors.get(what, 0.0))
        out[what] = (max(bound, REGIME_MARGIN * e32), e32, bound)
    return out
