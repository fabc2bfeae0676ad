"""Rebuilds tests/golden/shapelet_fwd_parent_bits.npz: the forward's outputs over tests/shapelet_fwd_bits_cases.py, bit for bit.

Run it ON AN MI355X WITH THE LIBRARY OF THE COMMIT BEFORE THE RING-WINDOW TWIN KERNELS (check that
commit out, build, then `python tests/gen_shapelet_fwd_parent_bits.py [out.npz]`): the fixture pins THAT library's bits, so that
tests/test_gpu_shapelet_fwd_bits.py can hold every later forward to them.  Both entry points are run and must already agree."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import speech_imagery_eeg_amd  # noqa: E402,F401
import shapelet_fwd_bits_cases as S  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "shapelet_fwd_parent_bits.npz")
    dev = torch.device("cuda:0")
    rec = {}
    for case in S.CASES:
        a, b = S.run(case, dev, "single"), S.run(case, dev, "bank")
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (case.name, k)
            assert not np.isnan(a[k]).any() if a[k].dtype != np.int32 else (a[k] >= 0).all(), (case.name, k)
        rec.update(S.stored(case, a))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **rec)
    print(f"wrote {out_path}: {len(rec)} arrays, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
