"""Shared cases of the faithfulness tests (tests/test_faithfulness_host.py, tests/test_gpu_faithfulness.py): score maps with every kind
of tie and bit pattern, requested k's at every edge, ragged lengths, and the sizes at which the select kernel changes its path.

The launch geometry of rank_threshold_kernel (csrc/ign_faithfulness.hip) is restated here: one workgroup of THREADS threads per
sample, UNROLL elements per thread and trip, so a trip of the block covers TRIP elements; KEY_PASSES byte passes over the key followed
by index_passes(n) byte passes over the flat index, where tied keys are cut."""
import numpy as np

THREADS = 1024          # RT_THREADS
UNROLL = 4              # RT_UNROLL
TRIP = THREADS * UNROLL
KEY_PASSES = 4
MAX_K = 32              # IGN_RANK_MAX_K

KINDS = ("continuous", "levels", "equal", "zeros", "special")


def index_passes(n):
    """byte passes over the index bits for a sample with n valid scores: the bit length of n - 1 in whole bytes"""
    return (max(int(n) - 1, 0).bit_length() + 7) // 8


def passes(n):
    return KEY_PASSES + index_passes(n)


def trips(n):
    return -(-int(n) // TRIP)


# (T, Cs): T*Cs of 1, a few, the first and second index byte, one below / at / above one trip, several trips, the third index byte
SIZES = [(1, 1), (1, 3), (7, 3), (256, 1), (257, 1), (TRIP - 1, 1), (TRIP, 1), (TRIP + 1, 1), (TRIP // 3, 3), (TRIP // 3 + 1, 3),
         (3001, 3), (65537, 1)]


def make_scores(kind, B, T, Cs, seed):
    rng = np.random.default_rng(seed)
    n = T * Cs
    if kind == "continuous":
        s = rng.standard_normal((B, n))
    elif kind == "levels":
        s = rng.integers(0, 3, (B, n)).astype(np.float64)
    elif kind == "equal":
        s = np.full((B, n), 0.5)
    elif kind == "zeros":
        s = np.where(rng.integers(0, 2, (B, n)) == 1, -0.0, 0.0)
    elif kind == "special":
        s = rng.standard_normal((B, n)).astype(np.float32)
        pool = np.array([np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45, 1e-39, 0.0, -0.0, 3.0, 3.0], np.float32)
        pool[3] = np.frombuffer(np.uint32(0xffc00001).tobytes(), np.float32)[0]       # a negative NaN with a payload
        hit = rng.random((B, n)) < 0.3
        s = np.where(hit, pool[rng.integers(0, len(pool), (B, n))], s)
        return np.ascontiguousarray(s.reshape(B, T, Cs), np.float32)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(s.reshape(B, T, Cs).astype(np.float32))


def make_lengths(B, T, ragged):
    """None, or int32 (B,): T, 0, 1, about half, beyond T (clamped), negative (clamped), in that order"""
    if not ragged:
        return None
    return np.array([T, 0, 1, (T + 1) // 2, T + 3, -2][:B], np.int32)


def make_k(n_b, nk, seed):
    """int32 (B, nk): per sample 0, 1, n - 1, n, above n, a negative value, duplicates and random ranks; with nk = 1 the samples walk
    through the edges instead"""
    rng = np.random.default_rng(seed)
    B = len(n_b)
    k = np.zeros((B, nk), np.int64)
    for b, n in enumerate(int(v) for v in n_b):
        edges = [0, 1, n - 1, n, n + 5, -3, n // 2, n // 2, 1, n]
        if nk == 1:
            k[b, 0] = edges[(b + seed) % 5]
        else:
            rnd = rng.integers(0, max(n, 1) + 1, nk)
            row = (edges + list(rnd))[:nk]
            k[b] = np.array(row)[rng.permutation(nk)]
    return k.astype(np.int32)


def rank_cases():
    """every (T, Cs) of SIZES with every kind of score, nk of 1 and 32, B walking 1..5, ragged lengths on every other case"""
    out, i = [], 0
    for T, Cs in SIZES:
        for kind in KINDS:
            for nk in (1, MAX_K):
                B = 1 + i % 5
                if T * Cs > 2 * TRIP * 3:
                    B = min(B, 2)                                # the long row: two samples are enough
                out.append(dict(T=T, Cs=Cs, kind=kind, nk=nk, B=B, ragged=(i % 2 == 1), seed=i))
                i += 1
    return out


def build(case):
    """-> (S (B,T,Cs) float32, k (B,nk) int32, lengths int32 (B,) or None, n_b (B,) int64)"""
    B, T, Cs = case["B"], case["T"], case["Cs"]
    S = make_scores(case["kind"], B, T, Cs, case["seed"])
    lengths = make_lengths(B, T, case["ragged"])
    n_b = np.full(B, T * Cs, np.int64) if lengths is None else np.clip(lengths.astype(np.int64), 0, T) * Cs
    return S, make_k(n_b, case["nk"], case["seed"]), lengths, n_b


def lexsort_rule(S, k, lengths=None):
    """The order restated with one lexsort: descending key, then ascending index -> (thr_key uint32, thr_idx int32)."""
    S = np.asarray(S, np.float32)
    B, T, Cs = S.shape
    thr_key = np.full(k.shape, 0xffffffff, np.uint32)
    thr_idx = np.full(k.shape, -1, np.int32)
    for b in range(B):
        n = T * Cs if lengths is None else min(max(int(lengths[b]), 0), T) * Cs
        u = S[b].reshape(-1)[:n].view(np.uint32).astype(np.int64)
        key = np.where(u >= 2 ** 31, 2 ** 32 - 1 - u, u + 2 ** 31)
        order = np.lexsort((np.arange(n), -key))
        for j in range(k.shape[1]):
            kk = min(max(int(k[b, j]), 0), n)
            if kk:
                thr_key[b, j], thr_idx[b, j] = key[order[kk - 1]], order[kk - 1]
    return thr_key, thr_idx


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.uint8), b.view(np.uint8))
