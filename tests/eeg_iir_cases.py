"""The case table of the IIR-stage tests (tests/test_eeg_iir_host.py, tests/test_gpu_eeg_iir.py) and its float64 references, computed
once per process and shared: inputs in the recipe of eeg_filterbank_cases.recordings (standard deviations of 5 to 80 uV on offsets of
+-2e4 uV), sfreq = 500 Hz everywhere.  The cases sit where the kernel can go wrong: fewer samples than lanes, T = P + 1, N = 64 and
65 (the chunk length goes 1 -> 3), an odd order, a partial last chunk, the maximum section count, a row count no tile divides, the
shards' row length and the longest row that fits."""
import functools

import numpy as np

from eeg_filterbank_cases import recordings

# label: (B, C, T, spec, P)        P is also what the spec's default pad gives, except where the case says otherwise
CASES = {
    "A_fewer_samples_than_lanes": (1, 1, 10, "notch=50", 9),                       # N = 28, idle lanes, Lc = 1
    "B_smallest_legal_row": (1, 1, 7, "hp=1,order=1", 6),                          # T = P + 1, a first-order section
    "C_one_sample_per_lane": (1, 2, 46, "lp=100,order=2", 9),                      # N = 64
    "D_first_rounded_chunk": (1, 2, 47, "lp=100,order=2", 9),                      # N = 65, Lc 2 -> 3
    "E_odd_order": (2, 3, 90, "hp=1,order=3", 12),                                 # a first-order section plus a biquad
    "F_full_chain": (2, 5, 300, "hp=0.5,lp=40,order=4,notch=50", 33),              # partial last chunk
    "G_eight_sections": (1, 3, 200, "hp=1,lp=45,order=8", 51),                     # the maximum section count
    "H_rows_vs_workgroup": (3, 7, 64, "notch=50", 9),                              # a row count no tile size divides
    "I_real_row_length": (2, 3, 1651, "hp=0.5,order=4,notch=50", 21),              # Lc = 27
    "J_longest_row": (1, 1, 8192 - 2 * 9, "notch=50", 9),                          # N = 8192; one more sample is IGN_E_TOOBIG
}


def I():
    import speech_imagery_eeg_amd  # noqa: F401
    from utils import eeg_iir
    return eeg_iir


@functools.lru_cache(maxsize=None)
def case(label):
    """-> dict(x, table, pad, g0, ns, ref64, scale): ref64 (B, C, T) is the float64 rule, scale (B, C, 1) is max_t |x - x[0]|; read-only"""
    m = I()
    B, C, T, spec, P = CASES[label]
    x = recordings(B, C, T)
    res = m.resolve_iir(f"{spec},pad={P}", T)
    assert res.pad == P == m.default_pad(res.sos), label                # the table's P is scipy's default for the design
    ref64 = m.iir_numpy(x, res.table, res.pad, res.g0)
    x64 = x.astype(np.float64)
    scale = np.abs(x64 - x64[..., :1]).max(axis=-1, keepdims=True)
    out = dict(x=x, table=res.table, pad=res.pad, g0=res.g0, ns=res.ns, ref64=ref64, scale=scale)
    for a in (x, res.table, ref64, scale):
        a.setflags(write=False)
    return out


def check_rows(label, y, ref64, scale):
    """The issue's bound, per row: |out - ref64| <= 2^-23 |ref64| + 1e-9 max|x - x[0]| -- one fp32 rounding of the result plus a
    term far above the order-of-evaluation distance in float64 (2e-13 with carries resolved one chunk after the other, 2e-11 with
    the kernel's scan across the lanes) and four orders below a float32 recurrence's error (4.7e-5).  -> the worst ratio of error to
    bound"""
    y = np.asarray(y, dtype=np.float64)
    assert y.shape == ref64.shape, (label, y.shape)
    assert np.isfinite(y).all(), label
    bound = 2.0 ** -23 * np.abs(ref64) + 1e-9 * scale
    err = np.abs(y - ref64)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"eeg_iir {label}: worst error / bound = {ratio:.4f}, max |err| / scale = {float((err / np.maximum(scale, 1e-300)).max()):.3e}")
    assert (err <= bound).all(), (label, ratio)
    return ratio
