"""The case table of the filter-bank tests (tests/test_eeg_filterbank_host.py, tests/test_gpu_eeg_filterbank.py) and its numpy
references, computed once per process and shared: inputs in the recipe of test_gpu_eeg_preprocess._recordings (standard deviations
of 5 to 80 uV, offsets of +-2e4 uV), Hamming band-pass taps and their quadrature pairs at sfreq 500 Hz, fp32-rounded."""
import functools

import numpy as np

SFREQ = 500.0
# label: (B, Cin, Tin, bands, M, q, Cout, Tout)
CASES = {
    "A_one_band": (2, 5, 64, ((8, 30),), 21, 1, 5, 64),                                     # nb = 1
    "B_crop_pad": (2, 5, 131, ((8, 13), (13, 30)), 41, 2, 7, 60),                           # zero electrodes inside each block, time crop
    "C_tile_crossing": (2, 33, 300, ((4, 8), (8, 13), (13, 30)), 101, 2, 33, 150),          # 99 channels: transpose tiles straddle bands
    "D_channel_crop": (2, 37, 200, ((8, 13), (13, 30), (30, 45)), 61, 3, 20, 67),           # Cout < Cin, q = 3
    "E_two_sweeps": (1, 3, 1651, ((8, 13), (13, 30)), 201, 1, 3, 1651),                     # Tv > 1280: second output sweep, fs reuse
    "F_eight_bands": (1, 2, 120, tuple((4 * i, 4 * i + 4) for i in range(1, 9)), 41, 2, 2, 60),   # nb at its limit
    "G_real_row": (2, 122, 1651, ((4, 8), (8, 13), (13, 30), (30, 45)), 201, 2, 122, 826),  # the shards' shape
}


def F():
    import speech_imagery_eeg_amd  # noqa: F401
    from utils import eeg_filter
    return eeg_filter


def recordings(B, C, T):
    rng = np.random.RandomState(B + C + T)
    return (rng.randn(B, C, T) * rng.uniform(5, 80, size=(B, C, 1)) + rng.uniform(-2e4, 2e4, size=(B, C, 1))).astype(np.float32)


def bank_taps(bands, M):
    """-> (H, G) fp32 (nb, M)"""
    f = F()
    H = np.stack([f.design_fir(SFREQ, lo, hi, M) for lo, hi in bands]).astype(np.float32)
    G = np.stack([f.design_quadrature(SFREQ, lo, hi, M) for lo, hi in bands]).astype(np.float32)
    return H, G


@functools.lru_cache(maxsize=None)
def case(label, envelope, edge="reflect"):
    """-> dict(x, H, G or None, q, Cout, Tout, Tv, Cv, nb, ref64, ref32, mask): the references are (B, Tout, nb * Cout), read-only"""
    f = F()
    B, Cin, Tin, bands, M, q, Cout, Tout = CASES[label]
    x = recordings(B, Cin, Tin)
    H, G = bank_taps(bands, M)
    G = G if envelope else None
    ref64, mask = f.pad_time(f.filterbank_numpy(x, H, G, q, edge, Cout, Tout), Tout)
    ref32, _ = f.pad_time(f.filterbank_numpy(x, H, G, q, edge, Cout, Tout, dtype=np.float32), Tout)
    for a in (x, H, ref64, ref32, mask):
        a.setflags(write=False)
    Td = -(-Tin // q)
    return dict(x=x, H=H, G=G, q=q, Cout=Cout, Tout=Tout, Tv=min(Td, Tout), Cv=min(Cin, Cout), nb=len(bands), ref64=ref64,
                ref32=ref32, mask=mask)
