"""Fixture of tests/test_eeg_preprocess_host.py: what scipy.signal designs and decimates, for the scipy-free designer and rule of
utils/eeg_filter.py to be compared against.  Needs scipy (the tests do not); no reference code is involved.

    python tests/golden/make_golden_eeg_preprocess.py        -> tests/golden/eeg_preprocess.npz
"""
import os

import numpy as np
from scipy import signal

HERE = os.path.dirname(os.path.abspath(__file__))
SFREQ = 500.0


def main():
    rng = np.random.RandomState(20)
    x = (rng.randn(2, 5, 131) * rng.uniform(5, 80, size=(2, 5, 1)) + rng.uniform(-200, 200, size=(2, 5, 1))).astype(np.float32)
    out = dict(
        sfreq=np.float64(SFREQ),
        taps_lowpass_61=signal.firwin(61, 45.0, window='hamming', fs=SFREQ),                          # low-pass at 45 Hz
        taps_bandpass_101=signal.firwin(101, [8.0, 30.0], window='hamming', pass_zero=False, fs=SFREQ),
        taps_highpass_201=signal.firwin(201, 4.0, window='hamming', pass_zero=False, fs=SFREQ),
        taps_decimate_q3=signal.firwin(20 * 3 + 1, 1.0 / 3, window='hamming'),                        # scipy.signal.decimate's own
        x=x,
    )
    for q in (2, 3):
        out[f"decimate_q{q}"] = signal.decimate(x.astype(np.float64), q, ftype='fir', zero_phase=True)
    path = os.path.join(HERE, "eeg_preprocess.npz")
    np.savez(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
