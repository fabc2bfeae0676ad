"""The shared cases of the artifact-stage tests (tests/test_eeg_artifact_host.py, tests/test_gpu_eeg_artifact.py), generated from
fixed seeds, and their references, computed once per process and read-only.  Rows are noise of 20 uV on per-row offsets of +-2e4 uV
unless a case says otherwise; the shapes are the smallest at which the kernels take another path: fewer samples than lanes, around
one wave, the CHISCO row, the row limit, ties, non-finite samples, every verdict, the neighbour weights."""
import functools

import numpy as np

U = 2.0 ** -24
KEYS = {
    "all": dict(clip=6.0, flat=0.01, noisy=8.0),
    "no_clip": dict(flat=0.01, noisy=8.0),
    "clip_only": dict(clip=6.0),
    "nothing": dict(),                                                   # the non-finite test alone
    "flat_zero": dict(clip=3.0, flat=0.0),                               # flat=0: only s = 0 is flat
}

# label: ((B, C, T), variants of KEYS that the device tests run)
CASES = {
    "A_fewer_samples_than_lanes": ((2, 3, 5), ("all", "nothing")),
    "B_63": ((1, 2, 63), ("all",)),
    "B_64_lower_median": ((1, 2, 64), ("all", "clip_only")),
    "B_65": ((1, 2, 65), ("all",)),
    "C_chisco_row": ((2, 122, 1651), ("all", "no_clip")),
    "D_2048": ((1, 2, 2048), ("all",)),
    "D_2049": ((1, 2, 2049), ("all",)),
    "E_row_limit": ((1, 2, 16384), ("all",)),
    "F_ties": ((1, 4, 257), ("all", "clip_only", "flat_zero")),
    "G_nonfinite": ((2, 6, 100), ("all", "nothing")),
    "H_verdicts_C1": ((5, 1, 200), ("all",)),
    "H_verdicts_C2": ((5, 2, 200), ("all",)),
    "H_verdicts_C7": ((5, 7, 200), ("all", "no_clip")),
    "H_verdicts_C8": ((5, 8, 200), ("all", "clip_only")),
    "I_neighbors": ((2, 8, 200), ("all", "no_clip")),
}
RUNS = [(label, v) for label, (_, vs) in CASES.items() for v in vs]


def A():
    import speech_imagery_eeg_amd  # noqa: F401
    from utils import eeg_artifact
    return eeg_artifact


def rows(rng, B, C, T):
    return (rng.randn(B, C, T) * 20.0 + rng.uniform(-2e4, 2e4, size=(B, C, 1))).astype(np.float32)


def _flatten(x, b, c):
    x[b, c] = x[b, c, 0]


def _noisy(x, b, c, gain=30.0):
    m = np.float32(np.median(x[b, c]))
    x[b, c] = (x[b, c] - m) * np.float32(gain) + m


@functools.lru_cache(maxsize=None)
def inputs(label):
    """-> (x (B,C,T) fp32, w (C,C) fp32 or None), read-only"""
    (B, C, T), _ = CASES[label]
    rng = np.random.RandomState(sum(map(ord, label)))
    x, w = rows(rng, B, C, T), None
    if label.startswith("A_"):
        x[1, 2, 3] += 900.0                                              # one spike among five samples
    elif label.startswith(("B_", "D_", "E_")):
        x[0, 1, ::7] += 400.0                                            # spikes for the clamp; row 0 is clean
    elif label.startswith("C_"):
        _flatten(x, 0, 17)                                               # a railed electrode
        _noisy(x, 0, 60)
        x[0, 101, 1650] = np.nan                                         # the last sample of a row
        x[0, 3, 100:104] += 900.0
        _noisy(x, 1, 121)                                                # the last electrode
        x[1, 0, 0] = np.inf
    elif label.startswith("F_"):
        x[0, 0] = rng.randint(-2, 3, size=T)                             # heavy ties
        x[0, 1] = np.where(rng.rand(T) < 0.5, 0.0, -0.0)                 # zeros of both signs
        x[0, 2] = -137.25                                                # constant: s = 0
    elif label.startswith("G_"):
        x[0, 0, 0] = np.nan
        x[0, 1, T - 1] = np.nan
        x[0, 2, 50] = np.inf
        x[0, 3, 51] = -np.inf
        x[0, 4, 10] += 900.0
        for c in range(C):                                               # sample 1: every row non-finite
            x[1, c, (13 * c) % T] = (np.nan, np.inf, -np.inf)[c % 3]
    elif label.startswith("H_"):
        # sample 0 clean; 1: flat and noisy together; 2: more than half flat (ref = 0); 3: exactly half flat (the LOWER median of an
        # even count is still 0); 4: noisy alone (C = 1: its own reference, good)
        if C == 1:
            _flatten(x, 1, 0)
            _flatten(x, 3, 0)
            _noisy(x, 4, 0)
        else:
            _flatten(x, 1, 0)
            _noisy(x, 1, C - 1)
            for c in range(C // 2 + 1):
                _flatten(x, 2, c)
            if C >= 7:
                x[2, C - 1, 4] = np.nan                                  # unrepaired and non-finite: zeros
            for c in range((C + 1) // 2):
                _flatten(x, 3, 2 * c)
            _noisy(x, 4, C // 2)
        x[0, 0, 9] += 900.0
    elif label.startswith("I_"):
        w = rng.rand(C, C).astype(np.float32)
        w[rng.rand(C, C) < 0.3] = 0.0                                    # zero weights
        np.fill_diagonal(w, 1e6)                                         # never read
        _noisy(x, 0, 2)
        _flatten(x, 0, 5)
        x[0, 6, 77] = np.nan
        w[5] = 0.0
        w[5, 2], w[5, 6] = 0.5, 2.0                                      # 5's positive-weight neighbours are all bad: fallback
        w[2, 0], w[2, 1] = 0.0, 0.0
        x[1, 0, 0] = np.nan
        x[1, 3, 20:23] += 900.0
    x.setflags(write=False)
    if w is not None:
        w.setflags(write=False)
    return x, w


@functools.lru_cache(maxsize=None)
def expected(label, variant):
    """-> dict(x, w, keys, y32, y64, verdict, stats, bound, scale): the fp32 rule, the float64 repair on the same fp32 inputs, the
    a-priori bound of the repaired elements (G + 3) u sum_j w_j |y_j - m_j| / sum_j w_j and, per sample, the largest centred
    amplitude among the good rows.  Read-only."""
    m = A()
    x, w = inputs(label)
    keys = KEYS[variant]
    y32, verdict, stats = m.artifact_numpy(x, w=w, **keys)
    y64, v64, s64 = m.artifact_numpy(x, w=w, repair64=True, **keys)
    assert np.array_equal(verdict, v64) and np.array_equal(stats, s64)
    B, C, T = x.shape
    bound, scale = np.zeros((B, C, T)), np.zeros(B)
    for b in range(B):
        good = np.flatnonzero(verdict[b] == 0)
        if not len(good):
            continue
        cen = np.abs(y64[b, good] - stats[b, good, 0:1].astype(np.float64))
        scale[b] = cen.max()
        for c in np.flatnonzero((verdict[b] >= 1) & (verdict[b] <= 3)):
            wj = np.ones(len(good)) if w is None else w[c, good].astype(np.float64)
            if not wj.sum() > 0:
                wj = np.ones(len(good))
            bound[b, c] = (len(good) + 3) * U * (wj[:, None] * cen).sum(0) / wj.sum()
    out = dict(x=x, w=w, keys=keys, y32=y32, y64=y64, verdict=verdict, stats=stats, bound=bound, scale=scale)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ shards with planted artifacts
def plant(X):
    """Artifacts in the shards of eeg_spatial_cases.write_shards, in place -> dict of what was planted: electrode 1 railed in every
    trial, electrode 4 at 30x noise in every third trial, one NaN (trial 5, electrode 2), 900 uV spikes in electrode 0 of four trials."""
    n, C, T = X.shape
    for i in range(n):
        X[i, 1] = X[i, 1, 0]
        if i % 3 == 0:
            m = np.float32(np.median(X[i, 4]))
            X[i, 4] = (X[i, 4] - m) * np.float32(30.0) + m
    X[5, 2, T // 2] = np.nan
    for i in (2, 7, 11, 13):
        X[i, 0, 5 + i] += 900.0
    return dict(flat=1, noisy=4, noisy_trials=[i for i in range(n) if i % 3 == 0], nan=(5, 2), spikes=(2, 7, 11, 13))
