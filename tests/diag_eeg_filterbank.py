"""Cost of the EEG filter bank (not a test): at B=256, Cin=122, Tin=2000 -> Tout=1000 (q=2), four bands (4:8, 8:13, 13:30, 30:45 Hz)
and 41 / 207 / 413 taps, the median of event-timed runs of ops.eeg_filterbank, plain and with the envelope, beside the yardstick a
user had before it: one ops.eeg_preprocess call per band plus torch.cat along the channel axis, timed in the same process.  That
composition reads the raw batch nb times and moves the output twice.  Bytes over HBM and FMAs (B*C*Td*M*nb, doubled with the
envelope) are computed from the shapes and set against the HBM peak (8.0 TB/s spec) and the plain v_fmac_f32 rate (39.3e12 FMA/s),
the columns of tests/diag_eeg_preprocess.py.  The GPU step is a child process under its own time limit.  No pass / fail threshold.

    python tests/diag_eeg_filterbank.py [--out profiles/eeg_filterbank.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
WARMUP, RUNS = 5, 41
SHAPE = dict(B=256, Cin=122, Tin=2000, q=2, Cout=122, Tout=1000)
BANDS = ((4.0, 8.0), (8.0, 13.0), (13.0, 30.0), (30.0, 45.0))
TAPS = (41, 207, 413)
HBM_PEAK, FMA_PEAK = 8.0e12, 39.3e12


def _median_ms(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return dict(median_ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1], runs=RUNS, warmup=WARMUP)


def _counts(M, envelope):
    """bytes over HBM and FMAs of one ops.eeg_filterbank call and of the composition, from the shapes"""
    B, C, Tin, q, Tout, nb = SHAPE["B"], SHAPE["Cin"], SHAPE["Tin"], SHAPE["q"], SHAPE["Tout"], len(BANDS)
    Td = -(-Tin // q)
    Tv = min(Td, Tout)
    raw, line, out = 4 * B * C * Tin, 4 * B * C * Tv, 4 * B * Tout * SHAPE["Cout"]
    return dict(bytes=raw + nb * (2 * line + out), bytes_raw_read=raw, bytes_workspace_write_plus_read=2 * nb * line,
                bytes_out_write=nb * out, bytes_composition=nb * (raw + 2 * line + out) + 2 * nb * out,
                fmas=B * C * Td * M * nb * (2 if envelope else 1))


def step_kernel():
    import numpy as np
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    from utils import eeg_filter as F
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, C, Tin, q = SHAPE["B"], SHAPE["Cin"], SHAPE["Tin"], SHAPE["q"]
    x = torch.randn(B, C, Tin, device=dev) * 30 + 500
    res = dict(hbm_peak_bytes_per_s=HBM_PEAK, fma_peak_per_s=FMA_PEAK)
    for M in TAPS:
        H = torch.from_numpy(np.stack([F.design_fir(500.0, lo, hi, M) for lo, hi in BANDS]).astype(np.float32)).to(dev)
        G = torch.from_numpy(np.stack([F.design_quadrature(500.0, lo, hi, M) for lo, hi in BANDS]).astype(np.float32)).to(dev)
        rows = [H[j].contiguous() for j in range(len(BANDS))]

        def composition():
            return torch.cat([ops.eeg_preprocess(x, h, decimate=q)[0] for h in rows], dim=2)

        # the yardstick first and last: its own spread within the run is the margin of the ratio
        comp = _median_ms(composition)
        plain = _median_ms(lambda: ops.eeg_filterbank(x, H, decimate=q))
        env = _median_ms(lambda: ops.eeg_filterbank(x, H, G, decimate=q))
        comp2 = _median_ms(composition)
        for k, envelope in ((plain, False), (env, True)):
            k.update(_counts(M, envelope))
            sec = k["median_ms"] * 1e-3
            k["share_of_hbm_peak"] = k["bytes"] / sec / HBM_PEAK
            k["share_of_fma_peak"] = k["fmas"] / sec / FMA_PEAK
            k["over_composition"] = k["median_ms"] / min(comp["median_ms"], comp2["median_ms"])
        env["over_plain_bank"] = env["median_ms"] / plain["median_ms"]
        res[f"composition_M{M}"] = comp
        res[f"composition_again_M{M}"] = comp2
        res[f"eeg_filterbank_M{M}"] = plain
        res[f"eeg_filterbank_envelope_M{M}"] = env
        res[f"bank_equals_composition_bitwise_M{M}"] = bool(torch.equal(ops.eeg_filterbank(x, H, decimate=q)[0], composition()))
    return res


STEPS = {"kernel": step_kernel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eeg_filterbank.json"))
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(STEPS[a.step]()))
        return
    res = dict(shape=SHAPE, bands=[list(b) for b in BANDS], taps=list(TAPS),
               yardstick="nb calls of ops.eeg_preprocess + torch.cat(dim=2); over_composition < 1 means the bank is faster; the "
                         "envelope does twice the FMAs of the composition it is set against")
    for name in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=300)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            res[name] = dict(failed=r.returncode, stderr=r.stderr[-2000:])
            break                                   # nothing more is started on the GPU after a failed step
        res[name] = json.loads(line[-1][7:])
        print(name, json.dumps(res[name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    if any("failed" in v for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
