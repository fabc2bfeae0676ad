"""Fixture of tests/test_eeg_iir_host.py: what scipy.signal designs (butter, iirnotch as second-order sections) and what its
sosfiltfilt returns, for the scipy-free designer and rule of utils/eeg_iir.py to be compared against.  Needs scipy (the tests do
not); no reference code is involved.

    python tests/golden/make_golden_eeg_iir.py        -> tests/golden/eeg_iir.npz
"""
import os

import numpy as np
from scipy import signal

HERE = os.path.dirname(os.path.abspath(__file__))
SFREQ = 500.0
ORDERS = (1, 3, 4, 5)
EDGE = dict(low=40.0, high=1.0)
NOTCH, Q = 50.0, 30.0


def default_padlen(sos):
    """sosfiltfilt's own default (scipy/signal/_signaltools.py)"""
    ntaps = 2 * sos.shape[0] + 1
    ntaps -= min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum())
    return 3 * int(ntaps)


def main():
    rng = np.random.RandomState(20)
    x = (rng.randn(2, 5, 131) * rng.uniform(5, 80, size=(2, 5, 1)) + rng.uniform(-200, 200, size=(2, 5, 1))).astype(np.float32)
    out = dict(sfreq=np.float64(SFREQ), x=x, orders=np.asarray(ORDERS), edge_low=np.float64(EDGE['low']),
               edge_high=np.float64(EDGE['high']), notch=np.float64(NOTCH), q=np.float64(Q))
    designs = {f"{kind}{n}": signal.butter(n, EDGE[kind], btype=kind, fs=SFREQ, output='sos') for kind in ('low', 'high') for n in ORDERS}
    b, a = signal.iirnotch(NOTCH, Q, fs=SFREQ)
    designs["notch"] = np.concatenate([b, a])[None]
    for name, sos in designs.items():
        out[f"sos_{name}"] = np.asarray(sos, dtype=np.float64)
        out[f"pad_{name}"] = np.int64(default_padlen(sos))
        out[f"y_{name}"] = signal.sosfiltfilt(sos, x.astype(np.float64), axis=-1)             # padtype='odd', the default padlen
    path = os.path.join(HERE, "eeg_iir.npz")
    np.savez(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
