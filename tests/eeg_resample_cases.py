"""The case table of the resampling-stage tests (tests/test_eeg_resample_host.py, tests/test_gpu_eeg_resample.py) and its float64
references, computed once per process and shared.  Rows carry offsets of +-2e4 uV under a signal of 30 uV standard deviation.  The
cases are the smallest shapes at which the kernel can go wrong: both edges inside one wave, more outputs than inputs, the 64/125 of
500 -> 256 Hz under both edge rules, more phases than a wave has lanes, a single phase, another phase length, the shortest legal row
and the longest one that fits the staging budget."""
import functools

import numpy as np

# label: (B, C, Tin, up, down, edge, half)
CASES = {
    "A_down_2_3": (2, 3, 50, 2, 3, "reflect", 10),
    "B_up_3_2": (2, 3, 50, 3, 2, "reflect", 10),                       # Lp = 21, Tout > Tin
    "C_64_125_zero": (1, 2, 301, 64, 125, "zero", 10),                 # Lp = 40, the mode scipy pins
    "D_chisco_row": (2, 122, 1651, 64, 125, "reflect", 10),            # Tout = 846
    "E_128_phases": (1, 2, 100, 128, 125, "reflect", 10),              # up > 64
    "F_one_phase": (1, 1, 97, 1, 2, "zero", 10),                       # pure decimation, odd Tin
    "G_half_4": (1, 2, 257, 64, 125, "reflect", 4),                    # Lp = 16
    "H_shortest_row": (1, 1, 32, 2, 3, "reflect", 10),                 # Tin = R + 1, R = Lp = 31
    "I_longest_row": (1, 1, 16261, 1, 2, "reflect", 10),               # 4 (Tin + 2*41 + 41) = 65536 bytes of LDS
}
PHASE_LEN = {"A_down_2_3": 31, "B_up_3_2": 21, "C_64_125_zero": 40, "D_chisco_row": 40, "E_128_phases": 21, "F_one_phase": 41,
             "G_half_4": 16, "H_shortest_row": 31, "I_longest_row": 41}


def R():
    import speech_imagery_eeg_amd  # noqa: F401
    from utils import eeg_resample
    return eeg_resample


def rows(B, C, T, seed):
    rng = np.random.RandomState(seed)
    return (rng.randn(B, C, T) * 30 + rng.uniform(-2e4, 2e4, size=(B, C, 1))).astype(np.float32)


def spec_text(up, down, edge, half):
    return f"ratio={up}/{down},half={half},edge={edge}"


@functools.lru_cache(maxsize=None)
def case(label):
    """-> dict(x, res, tab, up, down, hl, edge, Tout, ref64, ref32, scale): ref64 (B, C, Tout) is the float64 rule on the fp32 input
    and the fp32-rounded taps, ref32 its float32 numpy restatement, scale (B, C, 1) is max_t |x - x[0]|; read-only"""
    m = R()
    B, C, T, up, down, edge, half = CASES[label]
    x = rows(B, C, T, seed=T * 7 + up)
    res = m.resolve_resample(spec_text(up, down, edge, half), T)
    assert res.Lp == PHASE_LEN[label] and res.tab.dtype == np.float32, label
    ref64 = m.resample_numpy(x, res.tab, up, down, res.hl, edge)
    ref32 = m.resample_numpy(x, res.tab, up, down, res.hl, edge, dtype=np.float32)
    x64 = x.astype(np.float64)
    scale = np.abs(x64 - x64[..., :1]).max(axis=-1, keepdims=True)
    for a in (x, res.tab, res.taps, ref64, ref32, scale):
        a.setflags(write=False)
    return dict(x=x, res=res, tab=res.tab, up=up, down=down, hl=res.hl, edge=edge, Tout=res.Tout, ref64=ref64, ref32=ref32, scale=scale)
