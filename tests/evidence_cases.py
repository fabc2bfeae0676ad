"""Shared cases of the evidence-map tests (tests/test_evidence_host.py, tests/test_gpu_evidence.py): hand-placed match locations on
the smallest shapes at which the kernels can go wrong, and float64 restatements that share no array code with utils/evidence.py."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32

# (B, T, C): C below a wave, across one, above 128; T below, at, one past and two tiles past the kernel's 64-row time tile
SHAPES = [(3, 37, 5), (2, 64, 65), (2, 65, 130), (2, 129, 7)]
BANK = dict(Ks=(2, 3), Ls=(4, 19), strides=(1, 2))
# sum K = 530: with 4 electrode lanes (C <= 4) one chunk of the staged terms holds 512 features, so the chunk loop runs twice; with
# C = 65 (128 lanes, 16 features per chunk) it runs 34 times
BANK_WIDE = dict(Ks=(260, 270), Ls=(3, 5), strides=(1, 3))
CLASSES = (3, 39)


def make_case(B, T, C, N, Ks, Ls, strides, seed=0, scale=False):
    """-> dict(p, t, W, target, scale, Ks, Ls, strides, C, T): random p / W, and t random inside [0, Tw_g) except the hand-placed
    features of electrode 0 (and the last electrode): window 0 and the last window, two shapelets of one group overlapping, one
    feature with t = -1; targets differ per sample."""
    rng = np.random.default_rng(seed)
    ld = sum(Ks) * C
    p = rng.random((B, ld), dtype=np.float32)
    W = rng.standard_normal((N, ld)).astype(np.float32)
    t = np.empty((B, ld), np.int32)
    col0 = 0
    for K, L, s in zip(Ks, Ls, strides):
        Tw = (T - L) // s + 1
        t[:, col0:col0 + K * C] = rng.integers(0, Tw, size=(B, K * C))
        t[:, col0] = 0                                   # shapelet 0, electrode 0: the first window
        t[:, col0 + C - 1] = Tw - 1                      # shapelet 0, last electrode: the last window
        t[:, col0 + C] = min(1, Tw - 1)                  # shapelet 1, electrode 0: overlaps shapelet 0's window
        t[0, col0 + (K - 1) * C + C // 2] = -1           # no window (--mask_padding)
        col0 += K * C
    target = (np.arange(B) * 2 + 1) % N                  # differ per sample
    sc = (rng.random(B, dtype=np.float32) + np.float32(0.25)) if scale else None
    return dict(p=p, t=t, W=W, target=target.astype(np.int64), scale=sc, Ks=tuple(Ks), Ls=tuple(Ls), strides=tuple(strides), C=C, T=T)


def f32(x):
    """one float32 rounding of a float64 value: for one +, * of float32 operands evaluated in float64 this is the correctly
    rounded float32 result (53 >= 2 * 24 + 2 bits)"""
    return float(np.float32(x))


def evidence_loop(case, exact=False):
    """Direct triple loop over (b, s, c) and the features in the rule's order.  exact=False: every operation evaluated in float64 and
    rounded to float32 at once -- the rule's bits; exact=True: float64 throughout -- the value the rule approximates."""
    p, t, W, target, sc = case["p"], case["t"], case["W"], case["target"], case["scale"]
    C, T = case["C"], case["T"]
    B = p.shape[0]
    r = (lambda v: v) if exact else f32
    out = np.zeros((B, T, C), np.float64)
    for b in range(B):
        n = int(target[b])
        for c in range(C):
            terms, col0 = [], 0
            for K, L, stride in zip(case["Ks"], case["Ls"], case["strides"]):
                invL = 1.0 / L if exact else f32(1.0 / L)
                for k in range(K):
                    f = col0 + k * C + c
                    if t[b, f] >= 0:
                        terms.append((int(t[b, f]) * stride, L, r(r(float(W[n, f]) * float(p[b, f])) * invL)))
                col0 += K * C
            for s in range(T):
                acc = 0.0
                for start, L, v in terms:
                    if start <= s < start + L:
                        acc = r(acc + v)
                out[b, s, c] = r(acc * float(sc[b])) if sc is not None else acc
    return out


def cam_spread_loop(cam, R):
    cam = np.asarray(cam, np.float32)
    B, Tl = cam.shape
    out = np.zeros((B, Tl + R - 1), np.float64)
    invR = f32(1.0 / R)
    for b in range(B):
        for s in range(Tl + R - 1):
            acc = 0.0
            for tt in range(max(0, s - R + 1), min(s, Tl - 1) + 1):
                acc = f32(acc + float(cam[b, tt]))
            out[b, s] = f32(invR * acc)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def sum_bound(terms):
    """a-priori bound on |fp32 sum in any order - exact sum| of `terms` (plus three further roundings of the result):
    (n + 3) * 2^-24 * sum |terms|, evaluated in float64"""
    terms = np.asarray(terms, np.float64).ravel()
    return (terms.size + 3) * U * float(np.abs(terms).sum())
