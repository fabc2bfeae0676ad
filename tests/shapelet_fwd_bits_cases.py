"""Cases, inputs and the raw-ABI runner shared by tests/test_gpu_shapelet_fwd_bits.py and tests/gen_shapelet_fwd_parent_bits.py.

Every case is one length group at B = 3 (odd: the last row is exercised), C = 2.  The outputs of a case are what the forward writes:
p, dmin (B, K*C), tstar (B, K, C), zmu (B, K, C, 2), d (B, C, K, Tw) and, for cosine / pearson, xstat (B, C, Tw).  The fixture keeps
d in full for the named cases and as two position-weighted 32-bit checksums per (b, c, k) row for the sweep and the long rows
(any changed bit of a row changes its first checksum), which keeps the file at a few hundred KB."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

B, C, EPS = 3, 2, 0.8
L1, MSE, COS, PEARSON = 0, 1, 2, 3
RBF, LTS = 0x00, 0x10

Case = namedtuple("Case", "name T K L mode want_d x full")


def _c(name, T, K, L, mode=L1 | RBF, want_d=True, x="randn", full=True):
    return Case(name, T, K, L, mode, want_d, x, full)


CASES = [
    # the benchmark's four variants: TT = 15 / 13 / 11 / 8
    _c("bench_L100", 1000, 5, 100), _c("bench_L200", 1000, 5, 200), _c("bench_L300", 1000, 5, 300), _c("bench_L500", 1000, 5, 500),
    # window-count edges: Tw = 1, 63, 64, 65 (65: TT = 2 with lanes that hold no valid window)
    _c("tw1", 24, 5, 24), _c("tw63", 86, 5, 24), _c("tw64", 87, 5, 24), _c("tw65", 88, 5, 24),
    # tile edges
    _c("k7", 300, 7, 30),                               # tiles 5 + 2; TT = 5, J = 8, L % 8 = 6
    _c("k1", 200, 1, 9),                                # one tile of 1; L % 8 = 1
    _c("lmod4", 800, 5, 102, full=False),               # TT = 11, J = 4, L % 4 = 2
    _c("t1001", 1001, 5, 500),                          # T % 4 != 0: odd rows start off a 16-byte boundary, TT = 8
    _c("t203", 203, 5, 20),                             # ... at TT = 3
    _c("npass2", 1100, 5, 8, full=False),               # Tw = 1093 > 1024: two passes per row
    _c("nod_L300", 1000, 5, 300, want_d=False), _c("nod_small", 88, 7, 24, want_d=False),
    # gates and distances
    _c("lts_L100", 1000, 5, 100, L1 | LTS, full=False), _c("lts_k7", 300, 7, 50, L1 | LTS),
    _c("mse", 200, 5, 50, MSE | RBF), _c("cos", 200, 5, 50, COS | RBF), _c("pearson", 200, 7, 33, PEARSON | RBF),
    _c("mse_lts", 200, 5, 50, MSE | LTS),
    # first-index rule: x has period 50 and shapelet 0 is one period, so its best window occurs at t = 0, 50, 100, ...
    _c("periodic", 400, 5, 50, x="periodic"), _c("periodic_lts", 400, 5, 50, L1 | LTS, x="periodic", full=False),
] + [
    # every TT with tiles 5 + 2 + 1
    _c(f"tt{tt}", 64 * tt - 3 + 11, 8, 12, full=False) for tt in range(1, 17)
] + [
    # the first-index rule in a twin kernel (TT = 8): the recurring windows sit in different lanes
    _c("periodic_L500", 1000, 5, 500, x="periodic", full=False),
    # the LTS gate at the twin's TT = 13 / 11 / 8: these run the plain K_T = 5 kernels beside the twins (TT = 15: lts_L100)
    _c("lts_L200", 1000, 5, 200, L1 | LTS, full=False), _c("lts_L300", 1000, 5, 300, L1 | LTS, full=False),
    _c("lts_L500", 1000, 5, 500, L1 | LTS, full=False),
]
BY_NAME = {c.name: c for c in CASES}


def twin_tts():
    """The TT that have a twin kernel: FWD_TWIN_TTS of csrc/ign_shapelet_fwd.h."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "speech-imagery-eeg_amd", "csrc", "ign_shapelet_fwd.h")).read()
    mask = re.search(r"constexpr unsigned FWD_TWIN_TTS = ([^;]+);", src).group(1)
    return sorted(int(t) for t in re.findall(r"1u << (\d+)", mask))


def variants(case):
    """The (TT, KT, twin) kernels a case runs, and its passes per row: fwd_staging / launch_fwd_group of csrc/ign_abi.hip at
    stride 1 and the twin rule of shp_fwd_launch (K_T = 5, L1, RBF gate, one pass; blocks are always one wave)."""
    Tw = case.T - case.L + 1
    TT = min(16, (Tw + 63) // 64)
    npass = (Tw + 64 * TT - 1) // (64 * TT)
    out, k0 = [], 0
    for KT in (5, 2, 1):
        n = (case.K - k0) // KT
        if n > 0:
            out.append((TT, KT, KT == 5 and case.mode == L1 | RBF and npass == 1 and TT in twin_tts()))
            k0 += n * KT
    return out, npass


def inputs(case):
    """Seeded CPU inputs: xn (B, C, T), w (K, C, L), thr (K, C) or None."""
    g = torch.Generator().manual_seed(1234 + CASES.index(case))
    if case.x == "periodic":
        xn = torch.randn(B, C, 50, generator=g).repeat(1, 1, case.T // 50)
    else:
        xn = torch.randn(B, C, case.T, generator=g)
    w = torch.randn(case.K, C, case.L, generator=g)
    if case.x == "periodic":
        w[0] = xn[B - 1, :, :case.L]
    if case.mode & 0xf == PEARSON:
        w = w - w.mean(dim=-1, keepdim=True)            # the caller centres the shapelets
    thr = torch.rand(case.K, C, generator=g) * 2.0 if case.mode & LTS else None
    return xn.contiguous(), w.contiguous(), thr


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def run(case, dev, entry):
    """One forward through the raw C ABI; entry = "single" (ign_shapelet_fwd) or "bank" (ign_shapelet_fwd_bank, G = 1)."""
    from ign_hip import _lib
    xn, w, thr = [None if t is None else t.to(dev) for t in inputs(case)]
    K, L, T = case.K, case.L, case.T
    Tw = T - L + 1
    nan = float("nan")
    p = torch.full((B, K * C), nan, device=dev)
    dmin = torch.full((B, K * C), nan, device=dev)
    tstar = torch.full((B, K, C), -1, device=dev, dtype=torch.int32)
    zmu = torch.full((B, K, C, 2), nan, device=dev)
    d = torch.full((B, C, K, Tw), nan, device=dev) if case.want_d else None
    xstat = torch.full((B, C, Tw), nan, device=dev) if case.mode & 0xf >= COS else None
    h, s = _lib.lib(), _lib.stream()
    if entry == "single":
        rc = h.ign_shapelet_fwd(_vp(xn), _vp(w), _vp(thr), _vp(p), _vp(dmin), K * C, 0, _vp(tstar), _vp(zmu), _vp(d), _vp(xstat),
                                B, C, T, K, L, 1, EPS, case.mode, s)
    else:
        v1, i1 = ctypes.c_void_p * 1, ctypes.c_int * 1
        tab = lambda t: v1(None if t is None else t.data_ptr())
        rc = h.ign_shapelet_fwd_bank(_vp(xn), 1, tab(w), tab(thr) if thr is not None else None, _vp(p), _vp(dmin), K * C, i1(0),
                                     tab(tstar), tab(zmu), tab(d), tab(xstat), B, C, T, i1(K), i1(L), i1(1), EPS, case.mode, s)
    _lib.check(rc, f"{entry} {case.name}")
    torch.cuda.synchronize()
    out = dict(p=p, dmin=dmin, tstar=tstar, zmu=zmu)
    if d is not None:
        out["d"] = d
    if xstat is not None:
        out["xstat"] = xstat
    return {k: v.cpu().numpy() for k, v in out.items()}


def checksum(d):
    """(B, C, K, Tw) float32 -> (B, C, K, 2) uint32: wrapping sum of the bit patterns, and of the patterns times (2 t + 1)."""
    bits = np.ascontiguousarray(d).view(np.uint32).astype(np.uint64)
    pos = 2 * np.arange(d.shape[-1], dtype=np.uint64) + 1
    m = np.uint64(0xffffffff)
    return np.stack([bits.sum(-1) & m, ((bits * pos) & m).sum(-1) & m], axis=-1).astype(np.uint32)


def stored(case, out):
    """What the fixture keeps of a case's outputs, keyed '<case>/<array>'."""
    rec = {}
    for k, v in out.items():
        if k == "d":
            rec[f"{case.name}/d_ck"] = checksum(v)
            if not case.full:
                continue
        rec[f"{case.name}/{k}"] = v
    return rec
