"""Launch plan of the shapelet weight backward (ign_shapelet_bwd / ign_shapelet_bwd_bank), host side.  plan_bwd and
plan_bwd_strided (csrc/ign_abi.hip) derive from (B, C, T, K, L, stride) the positions per lane JJ, the chunks per shapelet, the
shapelets per block and the shapelet tiles, the block size, the window-axis chunk, the j-tiles of a long strided shapelet and
the batch slices nbs; nbs then selects the reduction kernel (csrc/ign_shapelet_bwd.hip).  This file

  * restates both plan functions and the reducers' slice bounds in Python (plan_bwd, reducer);
  * checks the restatement field by field against the built library (ign_shapelet_bwd_plan, ign_shapelet_bwd_workspace_bytes),
    over the case table and over a sweep of shapes around every switch point of the plan;
  * asserts that every row of tests/shapelet_bwd_plan_cases.py reaches the branch it is there for, and that the table as a whole
    covers every branch and every compiled instantiation at nbs >= 16 -- a retuned constant fails here instead of letting the
    GPU table quietly stop crossing its branches;
  * restates the float32 summation order of the L1 / RBF kernel and of the three reducers in numpy (grad_w_f32, reduce_f32) and
    shows, with a defect planted in the RESTATEMENT (never in the library), that the comparison of the GPU module -- grad_w
    against the float64 oracle at 1e-4 of the tensor's scale -- refuses each of them by at least ten times the tolerance.

Needs no GPU.  tests/diag_shapelet_bwd_plan.py prints the margins."""
import ctypes
import os

import numpy as np
import pytest

import shapelet_bwd_plan_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_TOOBIG = -1001, -1003
PLAN_FIELDS = ("JJ", "cpk", "kb", "nkt", "threads", "tc", "xs_len", "nbs", "njt", "lds")      # order of ign_shapelet_bwd_plan's out
PART_CAP = 256 << 20


# ------------------------------------------------------------------------------------------------------------ the plan
def _fill_tile(K, cpk):
    """shapelets per block: the tile that wastes the fewest lanes when kb*cpk is rounded up to whole waves, the smaller on ties"""
    best_kb, best_u = 1, -1.0
    kb = 1
    while kb <= K and kb * cpk <= 512:
        thr = (kb * cpk + 63) // 64 * 64
        ntile = (K + kb - 1) // kb
        u = K * cpk / (ntile * thr)
        if u > best_u + 1e-9:
            best_u, best_kb = u, kb
        kb += 1
    return best_kb


def plan_bwd(B, C, T_, K, L, stride=1):
    """plan_bwd / plan_bwd_strided -> dict of the plan's fields, what follows from them in the kernel (nch window chunks, the
    last chunk's length, the last tile's shapelets, the rows of every batch slice) and `capped`; or the refusal code."""
    Tw = (T_ - L) // stride + 1
    p = {}
    if stride > 1:
        JJ = 4
        cpk_all = (L + JJ - 1) // JJ
        p["njt"] = (cpk_all + 511) // 512
        p["cpk"] = (cpk_all + p["njt"] - 1) // p["njt"]
        p["kb"] = 1 if p["njt"] > 1 else _fill_tile(K, p["cpk"])
        budget_floor = 16 * 1024
    else:
        p["njt"] = 1
        best, best_eff = 0, -1.0
        for JJ in (8, 4):
            cpk = (L + JJ - 1) // JJ
            if cpk > 512:
                continue
            kb = max(1, min(K, 512 // cpk))
            threads = (kb * cpk + 63) // 64 * 64
            eff = kb * L / (threads * JJ)
            if JJ == 8:
                eff *= 1.10
            if eff > best_eff:
                best_eff, best = eff, JJ
        if not best:
            return E_TOOBIG
        JJ = best
        p["cpk"] = (L + JJ - 1) // JJ
        p["kb"] = _fill_tile(K, p["cpk"])
        budget_floor = 8 * 1024
    p["JJ"] = JJ
    p["nkt"] = (K + p["kb"] - 1) // p["kb"]
    p["threads"] = (p["kb"] * p["cpk"] + 63) // 64 * 64
    budget = max(budget_floor, p["threads"] // 64 * 5 * 1024)
    fixed = p["cpk"] * JJ + 16 * p["kb"] + 8
    tc_max = max(0, budget // 4 - fixed) // (stride + p["kb"])          # (a negative quotient loses to 2 * JJ below either way)
    tc_max = max(2 * JJ, tc_max // (2 * JJ) * (2 * JJ))
    nchunk = (Tw + tc_max - 1) // tc_max
    tc = (Tw + nchunk - 1) // nchunk
    tc = (tc + 2 * JJ - 1) // (2 * JJ) * (2 * JJ)
    p["tc"] = tc
    p["xs_len"] = (p["cpk"] * JJ + (tc - 1) * stride + 1 + 3) & ~3 if stride > 1 else (p["cpk"] * JJ + tc + 3) & ~3
    p["lds"] = (p["xs_len"] + p["kb"] * tc + 16 * p["kb"]) * 4
    if p["lds"] > 64 * 1024:
        return E_TOOBIG
    nbs = nbs0 = (B + 1) // 2
    while nbs > 1 and nbs * K * C * L * 4 > PART_CAP:
        nbs = (nbs + 1) // 2
    p["nbs"] = max(1, min(nbs, B))
    p["capped"] = p["nbs"] < max(1, min(nbs0, B))
    # what the kernel makes of it
    p["Tw"], p["n"], p["strided"] = Tw, K * C * L, stride > 1
    p["nch"] = (Tw + tc - 1) // tc
    p["last_chunk"] = Tw - (p["nch"] - 1) * tc
    p["last_tile"] = K - (p["nkt"] - 1) * p["kb"]
    p["slice_rows"] = [(B * bs // p["nbs"], B * (bs + 1) // p["nbs"]) for bs in range(p["nbs"])]
    p["rows_per_slice"] = {b1 - b0 for b0, b1 in p["slice_rows"]}
    return p


def reducer(nbs, route="group"):
    """Which kernel sums the nbs partials and how it cuts them up.  route="group": ign_launch_reduce_parts behind ign_shapelet_bwd
    (plain below 16 partials, reduce_parts_x4_kernel up to 128, reduce_parts_sliced_kernel above); route="bank":
    reduce_bank_kernel behind ign_shapelet_bwd_bank (plain below 16, the x4 order for any larger count).
    -> dict(kernel, per, slices [(p0, p1)], batches / tails per slice (x4: batches of 8 loads, then the remainder loop),
    empty_slices)."""
    assert route in ("group", "bank")
    if nbs < 16:
        return dict(kernel="plain", per=nbs, slices=[(0, nbs)], batches=[0], tails=[nbs], empty_slices=0)
    nsl = 16 if (route == "group" and nbs > 128) else 4
    per = (nbs + nsl - 1) // nsl
    slices = [(min(nbs, s * per), min(nbs, s * per + per)) for s in range(nsl)]
    x4 = nsl == 4
    return dict(kernel="x4" if x4 else "sliced", per=per, slices=slices,
                batches=[(p1 - p0) // 8 if x4 else 0 for p0, p1 in slices],
                tails=[(p1 - p0) % 8 if x4 else p1 - p0 for p0, p1 in slices],
                empty_slices=sum(p1 == p0 for p0, p1 in slices))


def describe(shape):
    """plan + reducers of a table row, flattened to the names the table's claims use"""
    p = plan_bwd(*shape)
    if not isinstance(p, dict):
        return dict(refused=True, rc=p)
    grp, bank = reducer(p["nbs"], "group"), reducer(p["nbs"], "bank")
    return dict(p, refused=False, reducer=grp["kernel"], bank=bank["kernel"], per=grp["per"], batches=grp["batches"],
                tails=grp["tails"], empty_slices=grp["empty_slices"])


# ------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("case", T.CASES, ids=T.IDS)
def test_every_row_reaches_its_branch(case):
    _, shape, mode, branch, claim = case
    got = describe(shape)
    assert {k: got.get(k) for k in claim} == claim, (branch, got)
    B, C, T_, K, L, stride = shape
    if not got["refused"]:
        rows = [b for b0, b1 in got["slice_rows"] for b in range(b0, b1)]
        assert rows == list(range(B))                                              # the slices tile the batch
        assert got["tc"] % (2 * got["JJ"]) == 0 and got["nch"] * got["tc"] >= got["Tw"] > (got["nch"] - 1) * got["tc"]
        assert got["njt"] * got["cpk"] * got["JJ"] >= L and got["kb"] * got["cpk"] <= got["threads"] <= 512


def test_the_table_covers_every_branch():
    d = {i: describe(s) for i, s, _, _, _ in T.CASES}
    live = {i: v for i, v in d.items() if not v["refused"]}
    nbs = {v["nbs"] for v in live.values()}
    assert nbs >= {1, 16, 17, 38, 128, 129, 130}
    # the three kernels of ign_launch_reduce_parts and both branches of reduce_bank_kernel, the latter also above 128 partials
    assert {v["reducer"] for v in live.values()} == {"plain", "x4", "sliced"}
    assert {(v["bank"], v["nbs"] > 128) for v in live.values()} == {("plain", False), ("x4", False), ("x4", True)}
    x4 = [v for v in live.values() if v["reducer"] == "x4"]
    assert any(not any(v["batches"]) for v in x4)                                  # remainder loop alone
    assert any(all(v["batches"]) and any(v["tails"]) for v in x4)                  # batches of 8, then a remainder
    assert any(all(v["batches"]) and not any(v["tails"]) for v in x4)              # batches of 8 alone
    assert any(len(set(zip(v["batches"], v["tails"]))) > 1 for v in x4)            # a shorter last slice
    sl = [v for v in live.values() if v["reducer"] == "sliced"]
    assert any(v["empty_slices"] for v in sl) and any(v["n"] % 16 for v in sl)
    assert any(len(v["rows_per_slice"]) > 1 for v in sl)
    assert any(v["capped"] for v in live.values())
    # shapelet tiles: a ragged one at kb > 1, several full ones, one shapelet per block
    assert any(v["kb"] > 1 and v["last_tile"] < v["kb"] for v in live.values())
    assert any(v["kb"] > 1 and v["nkt"] > 1 and v["last_tile"] == v["kb"] for v in live.values())
    assert any(v["kb"] == 1 and v["nkt"] > 1 for v in live.values())
    # positions per lane: both values, L below JJ, L no multiple of JJ for either, JJ = 8 at short and at forced length
    s1 = {i: v for i, v in live.items() if not v["strided"]}
    L_of = {i: s[4] for i, s, _, _, _ in T.CASES}
    assert any(v["JJ"] == 4 and L_of[i] < 4 for i, v in s1.items()) and any(v["JJ"] == 4 and L_of[i] % 4 for i, v in s1.items())
    assert any(v["JJ"] == 8 and L_of[i] % 8 for i, v in s1.items()) and any(v["JJ"] == 8 and L_of[i] < 100 for i, v in s1.items())
    assert any(2048 < L_of[i] <= 4096 for i in s1) and any(v["cpk"] == 512 and v["threads"] == 512 for v in s1.values())
    assert {v["threads"] for v in live.values()} >= {64, 320, 512}
    # window chunks: one, two with a ragged last one, many
    assert {1, 2, 7} <= {v["nch"] for v in live.values()}
    assert any(v["nch"] > 1 and v["last_chunk"] < v["tc"] for v in live.values())
    # the refusal, and the strided plans
    assert [i for i, v in d.items() if v["refused"]] == ["refused"] and d["refused"]["rc"] == E_TOOBIG
    assert any(v["strided"] and v["njt"] > 1 and v["nbs"] >= 16 for v in live.values())
    assert any(v["strided"] and v["njt"] == 1 and v["threads"] > 64 and v["nbs"] >= 16 for v in live.values())


def test_every_compiled_instantiation_and_both_gates_at_16_slices_or_more():
    seen, gates = set(), set()
    for i, shape, mode, _, _ in T.CASES:
        v = describe(shape)
        if v["refused"] or v["nbs"] < 16:
            continue
        dist, tie, strided = T.instantiation(shape, mode)
        seen.add((dist, tie, "strided" if strided else v["JJ"]))
        gates.add(mode & T.LTS)
    want = {(dist, tie, geo) for dist, tie in (("l1", False), ("l1", True), ("mse", False), ("cos", False), ("pearson", False))
            for geo in (4, 8, "strided")}
    assert seen == want, seen ^ want
    assert gates == {T.RBF, T.LTS}
    src = open(os.path.join(ROOT, "speech-imagery-eeg_amd", "csrc", "ign_shapelet_bwd.hip")).read()
    assert src.count("return shp_bwd_launch<") == 10 and src.count("return shp_bwd_strided_launch<") == 5


def test_the_teeth_rows_are_rows_of_the_table():
    assert set(T.TEETH.values()) <= set(T.IDS)
    for row in T.TEETH.values():
        _, shape, mode, _, _ = T.BY_ID[row]
        assert mode == T.L1 | T.RBF and shape[5] == 1                  # what grad_w_f32 restates


def test_jj_switch_points_at_the_driver_default_k():
    """K = 5: the choice between 4 and 8 positions per lane flips nine times up to L = 500 (listed: the first L of every run), and
    a single shapelet tile at K = 7 -- the backward has no 5 + 2 split, that is the forward's"""
    jj = [plan_bwd(3, 2, L + 50, 5, L)["JJ"] for L in range(1, 701)]
    flips = [(L, jj[L - 1]) for L in range(1, 701) if L == 1 or jj[L - 1] != jj[L - 2]]
    assert flips == [(1, 4), (49, 8), (97, 4), (153, 8), (201, 4), (257, 8), (305, 4), (357, 8), (409, 4), (449, 8)]
    assert [jj[L - 1] for L in (40, 56, 100, 200, 250, 260, 300, 500)] == [4, 8, 4, 8, 4, 8, 8, 8]
    p = plan_bwd(5, 3, 200, 7, 33)
    assert (p["kb"], p["nkt"]) == (7, 1)
    assert all((plan_bwd(3, 2, 200, 5, L)["kb"], plan_bwd(3, 2, 200, 5, L)["nkt"], plan_bwd(3, 2, 200, 5, L)["last_tile"]) == (2, 3, 1)
               for L in range(101, 114))


# ------------------------------------------------------------------------------------------------------------ the library
def _lib_or_skip():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    return _lib.lib()


def lib_plan(L, shape):
    """ign_shapelet_bwd_plan -> dict of PLAN_FIELDS, or the refusal code"""
    out = (ctypes.c_int * len(PLAN_FIELDS))(*([-7] * len(PLAN_FIELDS)))
    rc = L.ign_shapelet_bwd_plan(*shape, out)
    if rc:
        assert list(out) == [-7] * len(PLAN_FIELDS)                    # untouched on an error
        return rc
    return dict(zip(PLAN_FIELDS, out))


def _sweep():
    """shapes around every switch point: each L from 1 to 700 at K = 5 and K = 1, the long stride-1 shapelets up to the refusal,
    K from 1 to 45 at three lengths, strided plans up to five j-tiles, window axes from one to many chunks, batches around the
    reducer thresholds, and the 256 MB cap"""
    for L in range(1, 701):
        yield (3, 2, L + 37, 5, L, 1)
        yield (2, 3, 2 * L, 1, L, 1)
    for L in (1000, 2040, 2048, 2049, 2050, 3000, 4088, 4089, 4095, 4096, 4097, 4100, 5000):
        for K in (1, 2, 5):
            yield (2, 2, L + 9, K, L, 1)
    for K in range(1, 46):
        for L in (3, 12, 33):
            yield (3, 2, 120, K, L, 1)
    for L in (3, 10, 155, 310, 1799, 2048, 2049, 2400, 4096, 4097, 8992):
        for stride in (2, 7, 13):
            for K in (1, 2, 7):
                yield (2, 2, 2 * L + 100, K, L, stride)
    for T_ in (64, 500, 1000, 3000, 9000, 17984, 40000):
        yield (2, 2, T_, 3, 10, 1)
        yield (2, 2, T_, 5, 50, 3)
    for B in (1, 2, 3, 29, 30, 31, 32, 33, 75, 255, 256, 257, 258, 259, 1000):
        yield (B, 2, 64, 3, 8, 1)
    for B in (16, 31, 32, 33, 64, 256):
        yield (B, 122, 2048, 10, 2000, 1)
        yield (B, 122, 1000, 5, 500, 1)


def test_the_restatement_agrees_with_the_library_field_by_field():
    L = _lib_or_skip()
    n = 0
    for shape in list(_sweep()) + [c[1] for c in T.CASES]:
        want, got = plan_bwd(*shape), lib_plan(L, shape)
        if isinstance(want, dict):
            assert isinstance(got, dict) and got == {k: want[k] for k in PLAN_FIELDS}, (shape, got, want)
            B, C, T_, K, Ls, stride = shape
            assert L.ign_shapelet_bwd_workspace_bytes(*shape, 0) == want["nbs"] * K * C * Ls * 4
        else:
            assert got == want, (shape, got, want)
            assert L.ign_shapelet_bwd_workspace_bytes(*shape, 0) == 0
        n += 1
    assert n > 1500


def test_the_refused_shape_is_refused_by_the_query_and_both_entry_points_before_any_launch():
    """L = 4100 at stride 1: the query, the workspace size and both backward entry points refuse on the host -- the pointers are
    dummies, so a launch would not go unnoticed"""
    L = _lib_or_skip()
    shape = T.BY_ID["refused"][1]
    B, C, T_, K, Ls, stride = shape
    assert lib_plan(L, shape) == E_TOOBIG and b"no launch plan" in L.ign_last_error()
    assert L.ign_shapelet_bwd_workspace_bytes(*shape, 0) == 0
    pp = ctypes.c_void_p(16)
    assert L.ign_shapelet_bwd(pp, pp, pp, pp, pp, K * C, 0, pp, pp, pp, pp, pp, pp, pp, B, C, T_, K, Ls, stride, 1.0, 0, None) == E_TOOBIG
    assert b"ign_shapelet_bwd: no launch plan" in L.ign_last_error()
    one = ctypes.c_void_p * 1
    i1 = ctypes.c_int * 1
    tab = one(16)
    assert L.ign_shapelet_bwd_bank_workspace_bytes(1, B, C, T_, i1(K), i1(Ls), i1(stride), 0) == 0
    assert L.ign_shapelet_bwd_bank(pp, 1, tab, pp, pp, pp, K * C, i1(0), tab, tab, tab, tab, tab, tab, None, None, pp, B, C, T_, i1(K),
                                   i1(Ls), i1(stride), 1.0, 0, None) == E_ARG
    assert b"ign_shapelet_bwd_bank: group 0: no launch plan" in L.ign_last_error()
    # the query's own argument errors
    out = (ctypes.c_int * len(PLAN_FIELDS))()
    assert L.ign_shapelet_bwd_plan(2, 2, 10, 1, 11, 1, out) == E_ARG and L.ign_shapelet_bwd_plan(2, 2, 10, 1, 4, 0, out) == E_ARG
    assert L.ign_shapelet_bwd_plan(2, 2, 10, 1, 4, 1, None) == E_ARG


def test_the_query_is_declared_bound_and_leaves_the_abi_version_alone():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "ign_abi.h")).read()
    assert "int ign_shapelet_bwd_plan(int B, int C, int T, int K, int L, int stride, int* out);" in hdr
    assert f"#define IGN_SHAPELET_BWD_PLAN_FIELDS {len(PLAN_FIELDS)}\n" in hdr and "#define IGN_ABI_VERSION 1\n" in hdr
    res, args = _lib.SIGNATURES["ign_shapelet_bwd_plan"]
    assert res is ctypes.c_int and len(args) == 7


# ------------------------------------------------------------------------------------------------------------ float32 restatements
F32 = np.float32
DEFECTS = tuple(T.TEETH)
REDUCER_DEFECTS = tuple(d for d in DEFECTS if "reducer" in d)                     # planted in reduce_f32, the others in partials_f32


def _butterfly(v):
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


def _add_chunk_sum_f32(S, A, nthr):
    """S plus the sum of one staged chunk in the kernel's order: thread tid adds A[tid + u * nthr + i * 2 * nthr] (i, then u = 0, 1,
    ascending), the 64 lanes of a wave fold by the xor butterfly, the wave sums are added to S one after another.
    S (...), A (..., tc) float32 -> (...)"""
    tc = A.shape[-1]
    it = (tc + 2 * nthr - 1) // (2 * nthr)
    pad = np.zeros(A.shape[:-1] + (it * 2 * nthr,), F32)
    pad[..., :tc] = A
    pad = pad.reshape(A.shape[:-1] + (it * 2, nthr))
    part = np.zeros(A.shape[:-1] + (nthr,), F32)
    for i in range(it * 2):
        part = part + pad[..., i, :]
    waves = _butterfly(part.reshape(A.shape[:-1] + (nthr // 64, 64)))
    for wv in range(nthr // 64):
        S = S + waves[..., wv]
    return S


def partials_f32(xn, w, r, eps, plan, defect=None):
    """The nbs partial gradients (nbs, K, C, L) of the L1 / RBF backward at stride 1, float32 throughout, in the kernel's order: the
    coefficient A[b,k,c,t] = -(dl/dd) / L from float32 distances and row statistics; per batch slice, per row, per window chunk
    the lane's accumulators add A_t where x[b,c,t+j] > w[k,c,j], t ascending, and S adds the chunk's sum; the slice's partial is
    2 acc - S.  The forward quantities (d, arg-max, Z, mu) are plain float32 numpy, not the forward kernel's order."""
    x, w, r = np.asarray(xn, F32), np.asarray(w, F32), np.asarray(r, F32)
    B, C, T_ = x.shape
    K, _, L = w.shape
    Tw, tc, kb = plan["Tw"], plan["tc"], plan["kb"]
    eps = F32(eps)
    win = np.lib.stride_tricks.sliding_window_view(x, L, axis=2)                   # (B, C, Tw, L)
    d = np.empty((B, K, C, Tw), F32)
    for k in range(K):
        d[:, k] = np.abs(win - w[k][None, :, None, :]).mean(-1, dtype=F32)
    u = eps * d
    pp = np.exp(-(u * u))
    e = np.exp(pp)
    Z = e.sum(-1, keepdims=True, dtype=F32)
    mu = (e / Z * pp).sum(-1, keepdims=True, dtype=F32)
    hot = (np.arange(Tw) == pp.argmax(-1)[..., None]).astype(F32)
    g = r.reshape(B, K, C, 1)
    coef = g * (hot + e * (F32(1) / Z) * (pp - mu))
    A = -(coef * (-(F32(2) * eps * eps) * d * pp)) * (F32(1) / F32(L))            # (B, K, C, Tw)
    wcmp = w
    if defect == "ragged tile on its neighbour's weights":
        assert plan["last_tile"] == 1 and kb > 1
        wcmp = w.copy()
        wcmp[K - 1] = w[K - 2]
    parts = np.zeros((plan["nbs"], K, C, L), F32)
    chunks = list(range(0, Tw, tc))
    if defect == "last window chunk skipped":
        assert len(chunks) > 1
        chunks = chunks[:-1]
    for bs, (b0, b1) in enumerate(plan["slice_rows"]):
        if defect == "last batch slice loses its last row" and bs == plan["nbs"] - 1:
            assert b1 - b0 > 1
            b1 -= 1
        acc, S = np.zeros((K, C, L), F32), np.zeros((K, C), F32)
        for b in range(b0, b1):
            for t0 in chunks:
                Ac = np.zeros((K, C, tc), F32)
                n = min(tc, Tw - t0)
                Ac[..., :n] = A[b, :, :, t0:t0 + n]
                S = _add_chunk_sum_f32(S, Ac, plan["threads"])
                for t in range(n):
                    acc = acc + np.where(win[b, :, t0 + t][None] > wcmp, Ac[..., t:t + 1], F32(0))
        parts[bs] = F32(2) * acc - S[..., None]
    return parts


def reduce_f32(parts, route="group", defect=None):
    """the reduction over the batch slices in the order of `reducer(nbs, route)`: every slice of partials summed in ascending order
    from 0, the slice sums combined left to right"""
    nbs = parts.shape[0]
    red = reducer(nbs, route)
    slices = list(red["slices"])
    if defect == "x4 reducer skips its remainder loop":
        assert red["kernel"] == "x4" and any(red["tails"])
        slices = [(p0, p0 + 8 * nb) for (p0, _), nb in zip(slices, red["batches"])]
    elif defect == "sliced reducer drops its last non-empty slice":
        assert red["kernel"] == "sliced"
        last = max(i for i, (p0, p1) in enumerate(slices) if p1 > p0)
        slices[last] = (slices[last][0], slices[last][0])
    sums = []
    for p0, p1 in slices:
        s = np.zeros(parts.shape[1:], F32)
        for p in range(p0, p1):
            s = s + parts[p]
        sums.append(s)
    out = sums[0] if red["kernel"] == "plain" else np.zeros(parts.shape[1:], F32)
    if red["kernel"] != "plain":
        for s in sums:
            out = out + s
    return out


def grad_w_f32(case_id, defect=None, route="group"):
    _, shape, mode, _, _ = T.BY_ID[case_id]
    assert mode == T.L1 | T.RBF and shape[5] == 1
    xn, w, _, r = T.inputs(case_id)
    plan = plan_bwd(*shape)
    assert defect is None or defect in DEFECTS
    parts = partials_f32(xn.numpy(), w.numpy(), r.numpy(), T.EPS, plan, None if defect in REDUCER_DEFECTS else defect)
    return reduce_f32(parts, route, defect if defect in REDUCER_DEFECTS else None)


def grad_error(got, ref):
    """the figure the GPU module's comparison of grad_w judges (conftest.parity, kind="scale", floor 1e-12): max |got - ref| over
    the tensor's own scale; the comparison passes at <= GRAD_TOL"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), T.GRAD_FLOOR))


def _judge(label, got, ref, must_pass):
    """the GPU module's comparison itself; what it recorded is taken out of the ledger again (the ledger lists device errors)"""
    import conftest
    try:
        if must_pass:
            conftest.parity(label, got, ref, tol=T.GRAD_TOL, kind="scale", floor=T.GRAD_FLOOR)
        else:
            with pytest.raises(AssertionError):
                conftest.parity(label, got, ref, tol=T.GRAD_TOL, kind="scale", floor=T.GRAD_FLOOR)
    finally:
        for recs in conftest._LEDGER.values():
            recs.pop(label, None)
        for k in [k for k, v in conftest._LEDGER.items() if not v]:
            del conftest._LEDGER[k]


def teeth_margins(defect):
    """-> (error of the fault-free restatement, error with the defect planted), both over GRAD_TOL, and the two gradients"""
    row = T.TEETH[defect]
    _, shape, mode, _, _ = T.BY_ID[row]
    xn, w, thr, r = T.inputs(row)
    T.assert_no_ties(xn, w)
    ref = T.oracle(xn, w, thr, r, mode, shape[5])[2].numpy()
    good, bad = grad_w_f32(row), grad_w_f32(row, defect)
    return grad_error(good, ref) / T.GRAD_TOL, grad_error(bad, ref) / T.GRAD_TOL, good, bad, ref


@pytest.mark.parametrize("defect", DEFECTS)
def test_teeth_a_planted_defect_fails_the_gradient_comparison_tenfold(defect):
    clean, planted, good, bad, ref = teeth_margins(defect)
    print(f"{defect} at {T.TEETH[defect]}: fault-free {clean:.3f} x tol, planted {planted:.1f} x tol")
    _judge("restated grad_w", good, ref, must_pass=True)
    _judge(f"planted: {defect}", bad, ref, must_pass=False)
    assert clean <= 1.0 and planted >= 10.0, (clean, planted)


def test_the_bank_order_of_129_partials_differs_from_the_sliced_order_in_the_last_bits_only():
    """above 128 partials ign_shapelet_bwd_bank keeps the four-slice order while ign_shapelet_bwd takes sixteen slices: the two
    restated orders differ, and by rounding only -- why the GPU module compares both with float64 there instead of bit for bit"""
    a, b = grad_w_f32("nbs129", route="group"), grad_w_f32("nbs129", route="bank")
    assert np.any(a != b) and grad_error(a, b) < 1e-5
    assert np.array_equal(grad_w_f32("nbs17", route="group"), grad_w_f32("nbs17", route="bank"))
