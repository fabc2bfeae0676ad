"""The case table of the shapelet weight-backward launch-plan tests (tests/test_shapelet_bwd_plan_host.py restates the plan and
proves that every row reaches its branch; tests/test_gpu_shapelet_bwd_plan.py runs the rows against float64), and the seeded
inputs both use.  No torch at module level.

A row: (id, (B, C, T, K, L, stride), mode, branch, plan fields the row is there for).  `mode` is IGN_DIST_* | IGN_GATE_* |
IGN_TIE_EXACT of include/ign_abi.h.  The claimed fields are asserted from the restatement of plan_bwd / plan_bwd_strided
(csrc/ign_abi.hip) and, where the library is built, from ign_shapelet_bwd_plan itself; "reducer" / "bank" name the reduction
kernel of the per-group entry point (ign_launch_reduce_parts) / the branch of reduce_bank_kernel that the row's nbs selects."""
L1, MSE, COS, PEARSON = 0, 1, 2, 3
RBF, LTS, TIE = 0x00, 0x10, 0x20
EPS = 0.8
VAL_TOL = GRAD_TOL = 1e-4            # _close / _grad_close of tests/test_gpu_shapelet.py
GRAD_FLOOR = 1e-12
MODE_NAMES = {L1: "l1", MSE: "mse", COS: "cos", PEARSON: "pearson"}

S17 = (33, 2, 64, 3, 8, 1)           # nbs = 17 at JJ = 4
J17 = (33, 2, 100, 5, 60, 1)         # nbs = 17 at JJ = 8
T17 = (33, 2, 90, 3, 10, 3)          # nbs = 17, strided

CASES = [
    ("nbs1", (1, 2, 64, 3, 8, 1), L1, "one batch slice", dict(nbs=1, reducer="plain", bank="plain")),
    ("nbs16", (31, 2, 64, 3, 8, 1), L1, "lower edge of the x4 reducer: per = 4, no batch of 8",
     dict(nbs=16, reducer="x4", bank="x4", per=4, batches=[0, 0, 0, 0], tails=[4, 4, 4, 4])),
    ("nbs17", S17, L1, "x4, per = 5, last slice of 2", dict(JJ=4, nbs=17, reducer="x4", per=5, tails=[5, 5, 5, 2])),
    ("nbs38", (75, 2, 64, 3, 8, 1), L1, "x4, per = 10: one batch of 8 plus a remainder of 2",
     dict(nbs=38, reducer="x4", per=10, batches=[1, 1, 1, 1], tails=[2, 2, 2, 0])),
    ("nbs128", (256, 2, 64, 3, 8, 1), L1, "x4, all batches of 8",
     dict(nbs=128, reducer="x4", bank="x4", per=32, batches=[4, 4, 4, 4], tails=[0, 0, 0, 0])),
    ("nbs129", (257, 2, 40, 2, 6, 1), L1, "sliced reducer, per = 9, last slice empty, K*C*L = 24 is no multiple of 16",
     dict(nbs=129, reducer="sliced", bank="x4", per=9, empty_slices=1, n=24)),
    ("nbs130", (259, 2, 40, 3, 5, 1), L1, "sliced reducer, K*C*L = 30, odd split of rows over slices",
     dict(nbs=130, reducer="sliced", per=9, n=30, rows_per_slice={1, 2})),
    ("capped", (64, 122, 2048, 10, 2000, 1), L1, "partial buffer capped at 256 MB: nbs 32 -> 16, four rows per slice",
     dict(nbs=16, capped=True, reducer="x4", rows_per_slice={4})),
    ("ragged-tile", (3, 2, 150, 5, 101, 1), L1, "ragged shapelet tile: last tile holds one shapelet of kb = 2",
     dict(JJ=4, kb=2, nkt=3, last_tile=1)),
    ("kb20", (3, 2, 90, 40, 12, 1), L1, "twenty shapelets per block, two tiles", dict(kb=20, nkt=2, last_tile=20)),
    ("jj8-L260", (3, 2, 300, 1, 260, 1), L1, "JJ = 8 with L % 8 = 4", dict(JJ=8, cpk=33)),
    ("jj8-L60", J17, L1, "JJ = 8 at short L", dict(JJ=8, nbs=17, reducer="x4")),
    ("jj8-L96", (3, 2, 150, 5, 96, 1), L1, "last length of the first JJ = 8 run at K = 5", dict(JJ=8, cpk=12)),
    ("jj4-L97", (3, 2, 150, 5, 97, 1), L1, "first length of the next JJ = 4 run, L % 4 = 1", dict(JJ=4, cpk=25, kb=5)),
    ("L3", (3, 2, 40, 5, 3, 1), L1, "JJ = 4 with L < 4", dict(JJ=4, cpk=1)),
    ("L7", (3, 2, 40, 5, 7, 1), L1, "JJ = 4 with L % 4 != 0", dict(JJ=4, cpk=2)),
    ("two-chunks", (3, 2, 600, 5, 100, 1), L1, "two window chunks, the last one ragged: Tw = 501, tc = 256",
     dict(tc=256, nch=2, last_chunk=245)),
    ("seven-chunks", (3, 2, 3000, 3, 10, 1), L1, "seven window chunks", dict(nch=7)),
    ("L2050", (2, 2, 2100, 1, 2050, 1), L1, "L in (2048, 4096]: JJ = 8 is the only candidate", dict(JJ=8, cpk=257, threads=320)),
    ("L4096", (2, 2, 4100, 2, 4096, 1), L1, "the 512-thread block", dict(JJ=8, cpk=512, threads=512, kb=1, nkt=2)),
    ("refused", (2, 2, 4200, 1, 4100, 1), L1, "no plan above L = 4096 at stride 1", dict(refused=True)),
    ("strided-K7", (33, 2, 3100, 7, 155, 7), L1, "strided, nbs = 17, five waves", dict(JJ=4, njt=1, nbs=17, threads=320, reducer="x4")),
    ("strided-njt2", (33, 2, 3000, 1, 2400, 11), L1, "strided, two j-tiles per shapelet with nbs >= 16", dict(njt=2, kb=1, nbs=17)),
    # every compiled instantiation and both gates at nbs >= 16: mode variants of the small rows
    ("nbs17-tie", S17, L1 | TIE, "L1 IGN_TIE_EXACT, JJ = 4", dict(JJ=4, nbs=17)),
    ("nbs17-mse", S17, MSE, "MSE, JJ = 4", dict(JJ=4, nbs=17)),
    ("nbs17-cos", S17, COS, "cosine, JJ = 4", dict(JJ=4, nbs=17)),
    ("nbs17-pearson", S17, PEARSON, "pearson, JJ = 4", dict(JJ=4, nbs=17)),
    ("nbs17-lts", S17, L1 | LTS, "LTS gate, JJ = 4", dict(JJ=4, nbs=17)),
    ("jj8-tie", J17, L1 | TIE, "L1 IGN_TIE_EXACT, JJ = 8", dict(JJ=8, nbs=17)),
    ("jj8-mse", J17, MSE | LTS, "MSE under the LTS gate, JJ = 8", dict(JJ=8, nbs=17)),
    ("jj8-cos", J17, COS, "cosine, JJ = 8", dict(JJ=8, nbs=17)),
    ("jj8-pearson", J17, PEARSON, "pearson, JJ = 8", dict(JJ=8, nbs=17)),
    ("strided-l1", T17, L1, "strided L1", dict(JJ=4, nbs=17, strided=True)),
    ("strided-tie", T17, L1 | TIE, "strided L1 IGN_TIE_EXACT", dict(nbs=17, strided=True)),
    ("strided-mse", T17, MSE, "strided MSE", dict(nbs=17, strided=True)),
    ("strided-cos", T17, COS | LTS, "strided cosine under the LTS gate", dict(nbs=17, strided=True)),
    ("strided-pearson", T17, PEARSON, "strided pearson", dict(nbs=17, strided=True)),
    ("nbs129-lts", (257, 2, 40, 2, 6, 1), L1 | LTS, "sliced reducer under the LTS gate", dict(nbs=129, reducer="sliced")),
    ("nbs38-cos", (75, 2, 64, 3, 8, 1), COS, "cosine through the batched reducer loop", dict(nbs=38, reducer="x4")),
]
IDS = [c[0] for c in CASES]
BY_ID = {c[0]: c for c in CASES}
CAPPED_CHANNELS = (0, 121)           # the capped row's float64 reference: a weight gradient at channel c reads x[:, c] and g[:, :, c] only

# the planted defects of the host module: defect -> the row it is planted at
TEETH = {
    "x4 reducer skips its remainder loop": "nbs38",
    "sliced reducer drops its last non-empty slice": "nbs129",
    "last batch slice loses its last row": "nbs17",
    "ragged tile on its neighbour's weights": "ragged-tile",
    "last window chunk skipped": "two-chunks",
}


def instantiation(shape, mode):
    """what selects the compiled kernel of a row besides JJ -> (distance name, IGN_TIE_EXACT in effect, strided body)"""
    dist = mode & 0xf
    return MODE_NAMES[dist], bool(mode & TIE) and dist == L1, shape[5] > 1


def inputs(case_id):
    """-> xn (B,C,T), w (K,C,L), thr (1,K,C), r (B,K*C): seeded fp32 CPU tensors, tie-free the way _case_tensors of
    tests/test_gpu_input_grad.py makes them: the last mantissa bit is cleared in every sample and set in every weight (half an ulp
    at most, made before either side sees the inputs), so no sample is bit-equal to a weight and the sign(0) convention of the L1
    backward stays out of the comparison."""
    import torch
    _, (B, C, T, K, L, _), _, _, _ = BY_ID[case_id]
    gen = torch.Generator().manual_seed(7000 + IDS.index(case_id))
    xn = torch.randn(B, C, T, generator=gen)
    w = torch.randn(K, C, L, generator=gen)
    thr = torch.rand(1, K, C, generator=gen) * 2.0
    r = torch.randn(B, K * C, generator=gen)
    xn = (xn.view(torch.int32) & ~1).view(torch.float32)
    w = (w.view(torch.int32) | 1).view(torch.float32)
    return xn, w, thr, r


def assert_no_ties(xn, w):
    """no sample of a channel is bit-equal to a weight of that channel (stronger than "none that meet in a window")"""
    import numpy as np
    x, wn = xn.numpy(), w.numpy()
    for c in range(x.shape[1]):
        assert np.intersect1d(x[:, c].ravel(), wn[:, c].ravel()).size == 0, f"exact tie in channel {c}"


def oracle(xn, w, thr, r, mode, stride, device=None, chunk=None):
    """float64 autograd of sum(P * r) through oracle.ign_oracle -- the arithmetic of _oracle_bank of tests/test_gpu_input_grad.py,
    extended to d_min and to the cosine / pearson distances -> (P, Dmin, grad_w, grad_thr or None), float64 CPU tensors.
    `device`: where the float64 arithmetic runs (the larger rows take it on the GPU, as the 4.2 M-row LayerNorm case does)."""
    import torch
    from oracle import ign_oracle as O
    dev = device or torch.device("cpu")
    B, C, T = xn.shape
    K, _, L = w.shape
    Tw = (T - L) // stride + 1
    if chunk is None:                                     # the 5-D broadcast (B, chunk, K, C, L) stays below ~16 M elements
        chunk = max(1, min(Tw, (1 << 24) // max(1, B * K * C * L)))
    w64 = w.detach().to(dev, torch.float64).requires_grad_(True)
    t64 = thr.detach().to(dev, torch.float64).requires_grad_(True)
    d = O.window_distance(xn.detach().to(dev, torch.float64), w64, stride, mode & 0xf, chunk=chunk)
    P, D = O.lts_softmin_gate(d, t64) if mode & LTS else O.rbf_straight_through_max(d, EPS)
    grads = torch.autograd.grad((P * r.to(dev, torch.float64)).sum(), [w64] + ([t64] if mode & LTS else []))
    return P.detach().cpu(), D.detach().cpu(), grads[0].cpu(), (grads[1].cpu() if mode & LTS else None)
