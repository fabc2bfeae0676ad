"""Fixture of tests/test_eeg_resample_host.py: the low-pass scipy.signal.resample_poly designs (firwin with a Kaiser window, times
up) and what resample_poly returns on pivoted rows, for the scipy-free designer and rule of utils/eeg_resample.py to be compared
against.  Arrays only.  Needs scipy (the tests do not); no reference code is involved.

    python tests/golden/make_golden_eeg_resample.py        -> tests/golden/eeg_resample.npz
"""
import os

import numpy as np
from scipy import signal

HERE = os.path.dirname(os.path.abspath(__file__))
HALF, BETA = 10, 5.0
# name: (rows, Tin, up, down)
SHAPES = {"a": (3, 50, 2, 3), "b": (3, 50, 3, 2), "c": (2, 301, 64, 125), "e": (2, 100, 128, 125), "f": (2, 97, 1, 2)}


def main():
    rng = np.random.RandomState(31)
    out = dict(half=np.int64(HALF), beta=np.float64(BETA))
    for name, (rows, T, up, down) in SHAPES.items():
        x = (rng.randn(rows, T) * 30 + rng.uniform(-2e4, 2e4, size=(rows, 1))).astype(np.float32)
        mr = max(up, down)
        h = signal.firwin(2 * HALF * mr + 1, 1.0 / mr, window=('kaiser', BETA)) * up
        x64 = x.astype(np.float64)
        y = signal.resample_poly(x64 - x64[..., :1], up, down, axis=-1, window=('kaiser', BETA)) + x64[..., :1]
        out.update({f"x_{name}": x, f"up_{name}": np.int64(up), f"down_{name}": np.int64(down), f"h_{name}": h, f"y_{name}": y})
    path = os.path.join(HERE, "eeg_resample.npz")
    np.savez(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
