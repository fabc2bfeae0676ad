"""The case tables of the spatial-stage tests (tests/test_eeg_spatial_host.py, tests/test_gpu_eeg_spatial.py) and their float64
references, computed once per process and shared: inputs in the recipe of eeg_filterbank_cases.recordings (standard deviations of 5
to 80 uV, offsets of +-2e4 uV).  The bounds are a-priori bounds of an fmaf chain of Cin terms plus the two extra roundings (the
pivot subtraction and the final addition), u = 2^-24; none of them is a measured number."""
import functools

import numpy as np

from eeg_filterbank_cases import recordings

U = 2.0 ** -24

# label: (B, Cin, T, Cs, G, kind of W, gid or None)
APPLY_CASES = {
    "A_smallest": (1, 1, 4, 1, 1, "random", None),
    "B_car_odd_k": (2, 5, 64, 5, 1, "car", None),                       # Cin odd: the k padding
    "C_tile_crossing": (3, 33, 130, 7, 2, "random", (1, 0, 1)),         # crosses the 32-wide tile in c and in t, Cs < 32
    "D_wide_short": (2, 6, 31, 40, 1, "random", None),                  # Cs > Cin, T shorter than a tile
    "E_unused_group": (4, 70, 300, 64, 4, "random", (0, 1, 3, 1)),      # group 2 unused
    "F_real_row": (2, 122, 1651, 122, 3, "random", (2, 0)),             # the shards' row
}

# label: (B, C, T, G, gid or None)
GRAM_CASES = {
    "A_small": (3, 5, 64, 2, (1, 0, 1)),
    "B_empty_group": (4, 33, 130, 3, (2, 0, 2, 0)),                     # group 1 is empty
    "C_real_width": (2, 122, 300, 1, None),
}


def S():
    import speech_imagery_eeg_amd  # noqa: F401
    from utils import eeg_spatial
    return eeg_spatial


def weights(kind, G, Cs, Cin, seed):
    if kind == "car":
        assert Cs == Cin
        return np.broadcast_to(np.eye(Cin) - 1.0 / Cin, (G, Cs, Cin)).astype(np.float32)
    rng = np.random.RandomState(seed)
    return (rng.randn(G, Cs, Cin) / np.sqrt(Cin)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def apply_case(label):
    """-> dict(x, W, gid, y64, bound1, bound2, yc64): float64 product of the fp32 inputs and the two element-wise bounds, read-only"""
    B, Cin, T, Cs, G, kind, gid = APPLY_CASES[label]
    x = recordings(B, Cin, T)
    W = weights(kind, G, Cs, Cin, seed=B * 1000 + Cs)
    g = np.zeros(B, dtype=np.int32) if gid is None else np.asarray(gid, dtype=np.int32)
    x64, Wb = x.astype(np.float64), W.astype(np.float64)[g]
    y64 = np.einsum('bsc,bct->bst', Wb, x64)
    bound1 = (Cin + 2) * U * np.einsum('bsc,bct->bst', np.abs(Wb), np.abs(x64))
    xc = np.abs(x64 - x64[:, :, :1])
    bound2 = (Cin + 2) * U * np.einsum('bsc,bct->bst', np.abs(Wb), xc) + 2 * U * np.abs(y64).max(axis=-1, keepdims=True)
    yc64 = y64 - y64.mean(axis=-1, keepdims=True)
    out = dict(x=x, W=W, gid=None if gid is None else g, y64=y64, bound1=bound1, bound2=bound2, yc64=yc64)
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def check_apply(label, y):
    """both bounds of case `label` on an fp32 result y (B, Cs, T) -> (worst ratio to bound 1, worst ratio to bound 2)"""
    k = apply_case(label)
    y = np.asarray(y, dtype=np.float64)
    assert y.shape == k["y64"].shape, (label, y.shape)
    assert np.isfinite(y).all(), label
    e1 = np.abs(y - k["y64"])
    e2 = np.abs((y - y.mean(axis=-1, keepdims=True)) - k["yc64"])
    r1 = float((e1 / np.maximum(k["bound1"], 1e-300)).max())
    r2 = float((e2 / np.maximum(k["bound2"], 1e-300)).max())
    print(f"eeg_spatial {label}: error / bound 1 = {r1:.4f}, centred error / bound 2 = {r2:.4f}")
    assert (e1 <= k["bound1"]).all(), (label, "bound 1", r1)
    assert (e2 <= k["bound2"]).all(), (label, "bound 2", r2)
    return r1, r2


def identity_expectation(x):
    """What the rule gives for W = I, from the input alone: the chain adds exact zeros, so y = fl(fl(x - p) + p) -- which is x itself
    wherever x - p is exact in fp32 (always when the offset dominates the signal, Sterbenz; a row whose offset is small against its
    signal rounds x - p, and there the rule does not return x).  -> (y expected, mask of elements where x - p is exact)"""
    x = np.asarray(x, dtype=np.float32)
    p = x[..., :1]
    xc = x - p
    exact = xc.astype(np.float64) == x.astype(np.float64) - p.astype(np.float64)
    return xc + p, exact


@functools.lru_cache(maxsize=None)
def gram_case(label):
    """-> dict(x, gid, gram64, count, bound): the float64 Gram rule and 2 (n_g T + 8) u sum_{b,t} |z_i| |z_j|"""
    B, C, T, G, gid = GRAM_CASES[label]
    x = recordings(B, C, T)
    g = np.zeros(B, dtype=np.int32) if gid is None else np.asarray(gid, dtype=np.int32)
    gram64, count = S().gram_numpy(x, g, G)
    x64 = x.astype(np.float64)
    xc = x64 - x64[:, :, :1]
    z = np.abs(xc - xc.mean(axis=-1, keepdims=True))
    bound = np.zeros((G, C, C))
    for b in range(B):
        bound[g[b]] += z[b] @ z[b].T
    bound *= 2 * (count[:, None, None] * T + 8) * U
    out = dict(x=x, gid=None if gid is None else g, gram64=gram64, count=count, bound=bound)
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------- shards with subjects
def write_shards(root, n=24, C=6, T=64, subjects=3, seed=5):
    """X.npy / y.npy / subject.npy in the CHISCO contract: every subject's trials are a fixed mixing (condition number 4) of
    white sources, every electrode scaled to a standard deviation of 5 to 80 uV, on offsets of +-2e4 uV (the recipe of
    eeg_filterbank_cases.recordings, with a spatial covariance per subject).  -> (X, y, subject ids (non-dense on purpose))"""
    import os
    rng = np.random.RandomState(seed)
    ids = np.asarray([11, 40, 7, 93, 5][:subjects])
    subj = ids[np.arange(n) % subjects]
    rng.shuffle(subj)
    mix = {}
    for s in ids:
        q1, _ = np.linalg.qr(rng.randn(C, C))
        q2, _ = np.linalg.qr(rng.randn(C, C))
        m = q1 @ np.diag(np.geomspace(1.0, 4.0, C)) @ q2.T
        mix[s] = m / np.linalg.norm(m, axis=1, keepdims=True)              # unit variance per electrode, the subject's own correlations
    scale = rng.uniform(5, 80, size=(C, 1))
    X = np.stack([(mix[s] @ rng.randn(C, T)) * scale + rng.uniform(-2e4, 2e4, size=(C, 1)) for s in subj]).astype(np.float32)
    y = rng.randint(0, 39, size=n)
    np.save(os.path.join(root, "X.npy"), X)
    np.save(os.path.join(root, "y.npy"), y)
    np.save(os.path.join(root, "subject.npy"), subj)
    return X, y, subj
