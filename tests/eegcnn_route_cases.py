"""The case tables of the EEG-CNN route tests and a Python restatement of the dispatch rules they are built on
(tests/test_eegcnn_routes_host.py proves that every row reaches the route it names; tests/test_gpu_eegcnn_routes.py runs the rows
against float64 on an MI355X; tests/diag_eegcnn_routes.py records both in profiles/eegcnn_routes.json).  No torch at module level.

The block (models/eegcnn.py, csrc/ign_eegcnn.hip, csrc/ign_eegcnn_fused.hip) has a fast window, 2 <= k1 <= 125 and
k1 <= T <= 1024 (ops.bn1_data_stats + ops.bn1_fold, dwconv1d_wave_kernel, xcorr_kernel), and fallback routes around it.  The rows
below sit on the fallback routes and on the switch points between them and the window."""
E_ARG, E_UNSUP, E_TOOBIG = -1001, -1002, -1003

# ------------------------------------------------------------------------------------------------ bounds (none of them new)
DW_Y_TOL = DW_DX_TOL = 1e-5          # tests/test_gpu_baselines.py::test_dwconv1d_vs_torch
DW_DW_TOL = 2e-5
SUMSQ_TOL, SUMSQ_GRAD_TOL = 2e-5, 1e-4          # ::test_conv1_sumsq_vs_torch
LAG_TOL = 2e-6                       # ::test_window_gram_matrix_equals_brute_force, of the largest entry
CC_TOL = 1e-5                        # tests/test_gpu_eegcnn_fused.py::test_chan_contract_vs_float64, of scale
MODEL_TOL = 1e-4                     # conftest.parity(kind="scale") at its default
ZERO_GRAD_PARAMS = ("block1_bn1.weight", "block1_bn1.bias")      # removed by BatchNorm-2: true gradient < 1e-4 of the largest


def zero_grad_params(k1):
    """parameters whose true gradient vanishes up to BatchNorm's eps.  With one tap the temporal filter is a scale factor per
    filter, which BatchNorm-1 removes like BatchNorm-2 removes BatchNorm-1's affine map: block1_conv1.weight joins the list."""
    return ZERO_GRAD_PARAMS + (("block1_conv1.weight",) if k1 == 1 else ())

# ------------------------------------------------------------------------------------------------ csrc/ign_eegcnn.hip
XC_ROWS, XC_NA, XC_NB = 32, 4, 6
AC_LAGS, AC_ROWS = 128, 16
EG_MAXM = 124
WAVE_T_MAX = 1024
LDS_64K = 64 * 1024
G_THREADS, G_JJ, C1_FT = 256, 4, 8
ROW_TILE_MAX = 8184                  # models/eegcnn.py::_ROW_TILE_MAX = the largest T + k of dw_check


def xcorr_geometry(T, K):
    """xcorr_geometry: None where xcorr_kernel refuses (T, K), else its lanes per row, padded row, b-row length, lag tiles, LDS"""
    if T > 1024 or K > 128 or T < 1 or K < 1:
        return None
    T4 = (T + 3) & ~3
    NT = 1 if K <= 32 else 4
    l = 1
    while True:
        bl = 4 * l + 32 * NT + 8
        rpp = 256 // l
        if l >= T4 // 4 and rpp * T4 <= 256 * XC_NA and rpp * bl <= 256 * XC_NB:
            break
        if l == 256:
            return None
        l <<= 1
    return dict(lpr=l, T4=T4, BL=bl, NT=NT, rpp=rpp, lds=max(rpp * (T4 + bl), 4 * NT * 32) * 4)


def dw_check(T, k):
    """dw_check of the three ign_dwconv1d_* entry points: 0 or the refusal code"""
    if T <= 0 or k <= 0 or k > 1024:
        return E_ARG
    return E_TOOBIG if (2 * T + 2 * k + 16) * 4 > LDS_64K else 0


def dwconv_route(T, k, B=1):
    """ign_dwconv1d_fwd (forward and, flipped, the input gradient) and ign_dwconv1d_bwd_weight at rows of T samples, k taps"""
    rc = dw_check(T, k)
    if rc:
        return dict(refused=rc)
    if T <= WAVE_T_MAX:
        TT = 4 if T <= 256 else 8 if T <= 512 else 16
        fwd = dict(fwd="dwconv1d_wave_kernel", TT=TT, full_lanes=T == 64 * TT, tap_groups=k // 8, tap_tail=k % 8)
    else:
        fwd = dict(fwd="dwconv1d_kernel", TT=None, t_mod4=T % 4)
    if xcorr_geometry(T, k):
        dw = dict(dw="xcorr_kernel", slabs=(B + XC_ROWS - 1) // XC_ROWS)
    else:
        nbs = max(1, min(B, 32))
        rows = {(B * (s + 1)) // nbs - (B * s) // nbs for s in range(nbs)}
        dw = dict(dw="dwconv1d_bwd_w_kernel", slabs=nbs, rows_per_slab=rows, tap_slots=(k + 255) // 256)
    return dict(refused=0, **fwd, **dw)


def autocorr_route(T, K, R=1):
    """ign_autocorr_fwd -> kernel and the partial rows it writes (ign_autocorr_parts reserves 2 ceil(R / 16) either way)"""
    if K > AC_LAGS:
        return dict(kernel=None, refused=E_UNSUP)
    if xcorr_geometry(T, K):
        return dict(kernel="xcorr_kernel", refused=0, blocks=(R + XC_ROWS - 1) // XC_ROWS)
    xs_len = (((T + 3) & ~3) + AC_LAGS + 4 + 3) & ~3
    if 2 * xs_len * 4 > LDS_64K:
        return dict(kernel=None, refused=E_TOOBIG)
    nb = (R + AC_ROWS - 1) // AC_ROWS
    return dict(kernel="autocorr_kernel", refused=0, blocks=nb, last_block_rows=R - (nb - 1) * AC_ROWS)


def autocorr_sum_refuses(T, K):
    """ign_autocorr_sum_fwd answers IGN_E_UNSUP (before any launch) exactly when xcorr_geometry refuses"""
    return K > AC_LAGS or xcorr_geometry(T, K) is None


# ------------------------------------------------------------------------------------------------ csrc/ign_eegcnn_fused.hip
CW_TC, CW_MAX_BLOCKS = 64, 512


def cw_plan(B, T, aligned=True):
    """ign_chan_contract_bwd_weight: slices of 64 time steps, blocks (cw_blocks), kernel; `aligned`: du and x on 16 bytes"""
    slices = B * ((T + CW_TC - 1) // CW_TC)
    blocks = max(1, min(CW_MAX_BLOCKS, slices))
    return dict(slices=slices, blocks=blocks, grid_stride=slices > blocks,
                kernel="chan_contract_bwd_w_mfma_kernel" if T % 4 == 0 and aligned else "chan_contract_bwd_w_kernel")


# ------------------------------------------------------------------------------------------------ models/eegcnn.py
def conv1_sumsq_bwd_refuses(F1, k1):
    """ign_conv1_sumsq_bwd: one lane per (filter, four taps) of up to eight filters in a block of 256"""
    return ((k1 + G_JJ - 1) // G_JJ) * min(F1, C1_FT) > G_THREADS


def conv1_sumsq_max_taps(F1):
    return 4 * (G_THREADS // min(F1, C1_FT))


def gram_edges(k):
    """EEGcnn._window_gram: the edge terms come from ign_edge_lagprod_fwd up to 125 taps, from two torch GEMMs above"""
    return "edge_lagprod" if k - 1 <= EG_MAXM else "torch"


def bn1_route(T, k1, F1, momentum=0.1, track=True, variance_switch="gram", needs_grad=True):
    """BatchNorm-1 with batch statistics in EEGcnn._forward_hip -> "fold" (ops.bn1_data_stats + ops.bn1_fold), "gram/edge_lagprod" or
    "gram/torch" (the float64 quadratic form over _window_gram), "conv" (ops.conv1_sumsq) or "refused" (IgnError from forward)"""
    if T + k1 > ROW_TILE_MAX:
        return "refused"
    if variance_switch == "gram" and 2 <= k1 <= 125 and k1 <= T <= 1024 and (momentum is not None or not track):
        return "fold"
    if variance_switch == "gram" and 2 <= k1 <= 128 and T >= k1:
        return "gram/" + gram_edges(k1)
    if needs_grad and conv1_sumsq_bwd_refuses(F1, k1):
        return "refused"
    return "conv"


# ------------------------------------------------------------------------------------------------ the tables
# dwconv1d (B, C, T, k) -> the route fields the row is there for (asserted from dwconv_route), why
DWCONV_CASES = [
    ((2, 3, 256, 25), dict(fwd="dwconv1d_wave_kernel", TT=4, full_lanes=True, dw="xcorr_kernel"), "TT = 4, every lane full"),
    ((2, 3, 257, 25), dict(fwd="dwconv1d_wave_kernel", TT=8, dw="xcorr_kernel"), "first row length of TT = 8"),
    ((2, 3, 512, 8), dict(fwd="dwconv1d_wave_kernel", TT=8, full_lanes=True, tap_groups=1, tap_tail=0), "TT = 8 full, one tap group"),
    ((2, 3, 513, 7), dict(fwd="dwconv1d_wave_kernel", TT=16, tap_groups=0, tap_tail=7), "TT = 16, tail-only tap loop"),
    ((2, 3, 1024, 125), dict(fwd="dwconv1d_wave_kernel", TT=16, full_lanes=True, dw="xcorr_kernel"), "TT = 16 full: the longest wave row"),
    ((2, 2, 100, 1), dict(fwd="dwconv1d_wave_kernel", TT=4, tap_groups=0, tap_tail=1), "k = 1"),
    ((2, 2, 64, 24), dict(fwd="dwconv1d_wave_kernel", TT=4, tap_groups=3, tap_tail=0), "even k: pads 11 / 12"),
    ((2, 3, 1025, 25), dict(fwd="dwconv1d_kernel", t_mod4=1, dw="dwconv1d_bwd_w_kernel"), "generic kernels, T % 4 = 1"),
    ((2, 3, 1027, 4), dict(fwd="dwconv1d_kernel", t_mod4=3, dw="dwconv1d_bwd_w_kernel"), "generic kernels, T % 4 = 3"),
    ((2, 2, 1300, 125), dict(fwd="dwconv1d_kernel", t_mod4=0, dw="dwconv1d_bwd_w_kernel"), "generic kernels, two passes of 1024"),
    ((3, 2, 2050, 24), dict(fwd="dwconv1d_kernel", t_mod4=2, dw="dwconv1d_bwd_w_kernel"), "generic kernels, T % 4 = 2, even k"),
    ((33, 2, 1030, 6), dict(dw="dwconv1d_bwd_w_kernel", slabs=32, rows_per_slab={1, 2}), "B > 32: uneven batch slices"),
    ((1, 2, 1100, 300), dict(dw="dwconv1d_bwd_w_kernel", tap_slots=2), "k > 256: the second tap slot"),
    ((2, 3, 300, 129), dict(fwd="dwconv1d_wave_kernel", TT=8, dw="dwconv1d_bwd_w_kernel"), "k > 128 at T <= 1024: wave forward, fallback dw"),
    ((40, 2, 64, 130), dict(fwd="dwconv1d_wave_kernel", TT=4, dw="dwconv1d_bwd_w_kernel", slabs=32, rows_per_slab={1, 2}),
     "k > 128 with many rows, T < k"),
]

# autocorr (R, T, K)
AUTOCORR_CASES = [
    ((1, 1025, 1), dict(kernel="autocorr_kernel", blocks=1, last_block_rows=1), "smallest autocorr_kernel case"),
    ((16, 1026, 64), dict(kernel="autocorr_kernel", blocks=1, last_block_rows=16), "T > 1024, K = 64, one full block"),
    ((17, 1300, 125), dict(kernel="autocorr_kernel", blocks=2, last_block_rows=1), "one full block plus one row"),
    ((35, 2049, 128), dict(kernel="autocorr_kernel", blocks=3, last_block_rows=3), "largest K"),
    ((17, 1024, 125), dict(kernel="xcorr_kernel", blocks=1), "xcorr_kernel at the same K: the other side of the switch"),
]

# EEGcnn._window_gram (R, T, k, pl)
GRAM_CASES = [
    ((7, 1100, 25, 12), dict(kernel="autocorr_kernel", edges="edge_lagprod"), "T > 1024, edge kernel"),
    ((5, 1301, 124, 61), dict(kernel="autocorr_kernel", edges="edge_lagprod"), "T > 1024, largest edge kernel, even k"),
    ((3, 1500, 128, 63), dict(kernel="autocorr_kernel", edges="torch"), "torch edge Grams over autocorr_kernel"),
]

# conv1_sumsq (R, T, F1, k1): the shapes the model routes to it
SUMSQ_CASES = [
    ((3, 1500, 4, 25), "T > 1024"),
    ((2, 1100, 8, 125), "T > 1024"),
    ((4, 50, 3, 125), "T < k1"),
    ((5, 40, 4, 65), "T < k1"),
    ((3, 300, 2, 200), "k1 > 128"),
]

# chan_contract (B, Ci, Co, T), base offset of x and du in floats
CHAN_CASES = [
    ((70, 5, 3, 500), 0, dict(slices=560, blocks=512, grid_stride=True, kernel="chan_contract_bwd_w_mfma_kernel"), "grid-stride loop, MFMA"),
    ((140, 3, 2, 250), 0, dict(slices=560, blocks=512, grid_stride=True, kernel="chan_contract_bwd_w_kernel"), "grid-stride loop, T % 4 = 2"),
    ((70, 5, 3, 500), 1, dict(slices=560, blocks=512, grid_stride=True, kernel="chan_contract_bwd_w_kernel"),
     "T % 4 = 0 on a base one float off 16 bytes: the alignment fallback"),
]

# EEGcnn (B, C, T, k1, k2, F1, D, P1, P2), dropoutRate = 0; options; BatchNorm-1 route; why
MODEL_CASES = [
    ("long", (4, 9, 1100, 25, 25, 4, 2, 2, 4), {}, "gram/edge_lagprod", "long rows"),
    ("long-odd", (3, 5, 1301, 124, 8, 2, 3, 2, 5), {}, "gram/edge_lagprod", "long rows, odd T, even kernel, largest edge kernel"),
    ("T1024", (3, 5, 1024, 25, 25, 4, 2, 2, 4), {}, "fold", "last row length of the fast window"),
    ("T1025", (3, 5, 1025, 25, 25, 4, 2, 2, 4), {}, "gram/edge_lagprod", "first row length behind it"),
    ("k127", (6, 9, 200, 127, 25, 4, 2, 2, 4), {}, "gram/torch", "k1 in 126 .. 128: torch edge Grams"),
    ("k131", (6, 9, 200, 131, 25, 4, 2, 2, 4), {}, "conv", "k1 > 128"),
    ("T<k1", (8, 9, 40, 65, 25, 4, 2, 2, 4), {}, "conv", "T < k1"),
    ("T<pl", (8, 9, 20, 65, 25, 4, 2, 2, 4), {}, "conv", "T < left pad"),
    ("switch", (6, 9, 200, 31, 25, 4, 2, 2, 4), dict(variance_switch="conv"), "conv", "_BN1_VARIANCE = 'conv' inside the window"),
    ("cumulative", (6, 9, 200, 31, 25, 4, 2, 2, 4), dict(momentum=None), "gram/edge_lagprod", "momentum=None: cumulative average"),
    ("k1", (4, 5, 60, 1, 25, 4, 2, 2, 4), {}, "conv", "one tap: no lag to sum, ign_edge_lagprod_fwd takes k >= 2"),
]

# refusals: before any launch and before any state change
REFUSED_TAPS = dict(shape=(6, 9, 200, 131, 25, 8, 2, 2, 4), why="k1 = 131 at F1 = 8: no variance gradient")
REFUSED_ROW = dict(shape=(1, 2, 9000, 25, 25, 4, 2, 2, 4), why="T = 9000 does not fit the LDS row tiles")

# EEGcnn._shifted_sums (T, k), pl = (k - 1) // 2; the last two are rows shorter than the left pad
SHIFTED_SUMS_CASES = [(200, 31), (40, 65), (64, 64), (10, 1), (9, 2), (33, 65), (32, 65), (5, 8), (20, 65), (3, 9)]
SHIFTED_SUMS_TOL = 1e-12


def model_kernels(shape, opts=None):
    """what one training step of a MODEL_CASES row launches, from the restatements: BatchNorm-1 route, lag-sum kernel, the depthwise
    kernels of block 1 (T, k1) and block 2 (T // P1, k2), the plan of the electrode contraction's weight gradient"""
    B, C, T, k1, k2, F1, D, P1, P2 = shape
    opts = opts or {}
    route = bn1_route(T, k1, F1, momentum=opts.get("momentum", 0.1), variance_switch=opts.get("variance_switch", "gram"))
    out = dict(bn1=route, block1=dwconv_route(T, k1, B), block2=dwconv_route(T // P1, k2, B), chan1=cw_plan(B, T))
    if route.startswith("gram"):
        out["lag_sums"] = autocorr_route(T, k1, B * C)["kernel"]
    return out
