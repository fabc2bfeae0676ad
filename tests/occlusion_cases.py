"""Shared cases of the occlusion tests (tests/test_occlusion_host.py, tests/test_gpu_occlusion.py): time grids at every edge of the grid
formula, electrode counts at which a lane's quad ends inside a row, the three kinds of electrode groups, ragged lengths, fills and
batches with every special bit pattern, and the chunk edges of the patch range -- plus a second, loop-per-cell restatement of the two
rules of utils/occlusion.py."""
import numpy as np

from faithfulness_cases import make_lengths, make_scores, same_bits  # noqa: F401

MAX_COVER = 64          # IGN_OCC_MAX_COVER

# (T, window, stride): one step; a window of one; overlapping, touching and strided windows on a short row; (12, 20, 4): the window
# is clamped to T; (37, 8, 3): (T - W) % S != 0, the last window hangs over the end; (129, 64, 1): ceil(W / S) reaches MAX_COVER
GRIDS = [(1, 0, 0), (1, 1, 1), (7, 3, 1), (7, 3, 2), (7, 3, 3), (12, 5, 2), (12, 12, 12), (12, 20, 4), (37, 8, 3), (65, 16, 16),
         (129, 64, 1)]
CHANNELS = (1, 3, 5, 64, 65, 130)
GROUPS = ("all", "each", "irregular")


def grid_of(T, window, stride):
    """the grid formula restated -> (W, S, nt)"""
    W = T if window <= 0 else min(window, T)
    S = W if stride <= 0 else stride
    assert 1 <= S <= W
    return W, S, (T - W + S - 1) // S + 1


def make_gid(kind, C):
    """-> (gid int32 (C,), G).  "irregular": a few uneven groups, one group id that no electrode carries and -- from C = 3 on -- one
    group of a single electrode."""
    if kind == "all":
        return np.zeros(C, np.int32), 1
    if kind == "each":
        return np.arange(C, dtype=np.int32), C
    if C < 3:
        return np.full(C, 2, np.int32), 3                          # groups 0 and 1 are empty
    gid = np.where(np.arange(C) % 3 == 0, 0, 3).astype(np.int32)   # group 1 is empty
    gid[C - 1] = 2                                                 # group 2 is one electrode
    return gid, 4


def make_fill(B, C, seed):
    rng = np.random.default_rng(1000 + seed)
    f = (rng.standard_normal((B, C)) + 10.0).astype(np.float32)
    flat = f.reshape(-1).view(np.uint32)
    flat[0] = 0x80000000                                           # -0.0
    if flat.size > 1:
        flat[1] = 0x7fc00123                                       # a NaN with a payload
    if flat.size > 2:
        flat[2] = 0x7f800000                                       # inf
    return f


def chunk_edges(P):
    """(p0, count): everything, the first patch, the last patch, and a split P = a + b with b < a"""
    out = [(0, P), (0, 1), (P - 1, 1)]
    if P >= 3:
        a = P // 2 + 1
        out += [(0, a), (a, P - a)]
    return out


def make_drop(B, P, seed):
    """finite drops of mixed sign and magnitude (cancellation, subnormal results, -0.0): what a score difference can be"""
    rng = np.random.default_rng(2000 + seed)
    d = (rng.standard_normal((B, P)) * 10.0 ** rng.integers(-3, 4, (B, P))).astype(np.float32)
    pool = np.array([0.0, -0.0, 1e-39, -1e-39, 1e-45, 3.0, -3.0, 1e30, -1e30, 16777216.0, 1.0], np.float32)
    hit = rng.random((B, P)) < 0.25
    return np.where(hit, pool[rng.integers(0, len(pool), (B, P))], d).astype(np.float32)


def occlusion_cases():
    """every grid with a walk through the electrode counts, the groups, the lengths, the fill and B = 1..5; every (C, groups) pair and
    every (groups, ragged, fill) combination is met"""
    out, i = [], 0
    for T, window, stride in GRIDS:
        for j, C in enumerate(CHANNELS):
            for groups in GROUPS:
                if T == 129 and C > 5 and not (C == 65 and groups == "all"):
                    continue                                        # the long overlapping grid (66 windows, 64 over a step): small C
                out.append(dict(T=T, window=window, stride=stride, C=C, groups=groups, B=1 + i % 5, ragged=(i // 3) % 2 == 1,
                                fill=(i // 2) % 2 == 1, seed=i))
                i += 1
    return out


def build(case):
    """-> (x (B,T,C) float32, gid, G, lengths or None, fill or None)"""
    B, T, C = case["B"], case["T"], case["C"]
    x = make_scores("special", B, T, C, case["seed"])
    gid, G = make_gid(case["groups"], C)
    return x, gid, G, make_lengths(B, T, case["ragged"]), (make_fill(B, C, case["seed"]) if case["fill"] else None)


# ---------------------------------------------------------------- the rules restated cell by cell
def occlude_loops(x, p0, count, gid, G, window, stride, fill=None, lengths=None):
    xb = np.ascontiguousarray(x, np.float32).view(np.uint32)
    B, T, C = xb.shape
    W, S, nt = grid_of(T, window, stride)
    fb = None if fill is None else np.ascontiguousarray(fill, np.float32).view(np.uint32)
    out = np.empty((B * count, T, C), np.uint32)
    members = [[c for c in range(C) if gid[c] == g] for g in range(G)]
    for b in range(B):
        n = T if lengths is None else min(max(int(lengths[b]), 0), T)
        for q in range(count):
            i, g = divmod(p0 + q, G)
            row = out[b * count + q]
            row[:] = xb[b]
            for t in range(i * S, min(i * S + W, n)):
                for c in members[g]:
                    row[t, c] = 0 if fb is None else fb[b, c]
    return out.view(np.float32)


def spread_loops(drop, gid, G, window, stride, T, lengths=None):
    D = np.ascontiguousarray(drop, np.float32)
    B, C = D.shape[0], len(gid)
    W, S, nt = grid_of(T, window, stride)
    out = np.zeros((B, T, C), np.float32)
    for b in range(B):
        n = T if lengths is None else min(max(int(lengths[b]), 0), T)
        for t in range(n):
            over = [i for i in range(nt) if i * S <= t < i * S + W]                 # ascending
            for c in range(C):
                s = D[b, over[0] * G + gid[c]]
                for i in over[1:]:
                    s = np.float32(s + D[b, i * G + gid[c]])
                out[b, t, c] = np.float32(s * (np.float32(1.0) / np.float32(len(over))))
    return out
