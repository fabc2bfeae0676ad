"""Cost of the rational resampling stage (not a test): ops.eeg_resample (ign_eeg_resample_nct) at the CHISCO shape
(256, 122, 1651) for 64/125 and at (256, 122, 2000) for 1/2, beside the yardstick the stage was sized against -- ops.eeg_preprocess
with decimate=2 and 41 taps at (256, 122, 2000): about the same 40 multiply-adds per output and 1000 outputs per row, plus a
statistics sweep and a transpose that this stage does not have, minus the second LDS read per multiply-add that its per-lane taps
cost -- and beside the torch composition of the same arithmetic (zero-stuff by `up`, depthwise F.conv1d with stride `down`, crop).
All timed in one process with device events around windows of back-to-back calls, the candidates alternating window by window.
Multiply-adds and bytes over HBM (one read of the batch, one write of the result) are counted from the shapes and set against the
peaks.  The GPU step is a child process under its own time limit.

    python tests/diag_eeg_resample.py [--out profiles/eeg_resample.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
WARMUP, WINDOW, ROUNDS = 5, 40, 7
SHAPES = {"chisco_64_125": dict(B=256, C=122, T=1651, spec="rate=256"), "decimate_1_2": dict(B=256, C=122, T=2000, spec="ratio=1/2")}
YARDSTICK = dict(B=256, C=122, T=2000, decimate=2, taps=41)
HBM_PEAK, VALU_F32_PEAK, LDS_DWORDS_PER_S = 8.0e12, 157.3e12, 256 * 32 * 2.4e9       # ds_read_b32: 32 dwords per clock and CU


def _windows(fns, warmup=WARMUP, window=WINDOW, rounds=ROUNDS):
    """{name: fn} -> {name: per-call ms, median over `rounds` windows of `window` calls}, the fns alternating window by window"""
    import torch
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(window):
                fn()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) / window)
    out = {}
    for name, t in ts.items():
        t.sort()
        out[name] = dict(median_ms=t[len(t) // 2], min_ms=t[0], max_ms=t[-1], windows=rounds, calls_per_window=window, warmup=warmup)
    return out


def step(which):
    """which='kernel': the stage and its yardstick; which='torch': the torch composition alone (soft: its zero-stuffed rows are `up`
    times the batch and its convolution has thousands of taps)"""
    import numpy as np
    import torch
    import torch.nn.functional as F
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    from utils.eeg_filter import parse_eeg_preprocess, resolve
    from utils.eeg_resample import resample_numpy, resolve_resample
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    fns, slow, meta, keep = {}, {}, {}, {}
    for name, s in SHAPES.items():
        B, C, T = s["B"], s["C"], s["T"]
        x = torch.randn(B, C, T, device=dev) * 30 + torch.empty(B, C, 1, device=dev).uniform_(-2e4, 2e4)
        st = resolve_resample(s["spec"], T)
        tab = torch.from_numpy(st.tab).to(dev)
        y = torch.empty(B, C, st.Tout, device=dev)
        kw = dict(up=st.up, down=st.down, half_len=st.hl, edge=st.edge)
        fns[name] = lambda x=x, tab=tab, y=y, kw=kw: ops.eeg_resample(x, tab, out=y, **kw)
        # torch: zero-stuff, depthwise convolution with the taps reversed (conv1d correlates), stride down, crop to Tout; zero edge
        h = torch.from_numpy(st.tab.T.reshape(-1)[:2 * st.hl + 1].copy()).to(dev)
        w = h.flip(0).reshape(1, 1, -1)

        def torch_form(x=x, w=w, st=st, B=B, C=C, T=T):
            u = x - x[..., :1]
            z = torch.zeros(B * C, 1, T * st.up, device=x.device)
            z[:, 0, ::st.up] = u.reshape(B * C, T)
            out = F.conv1d(z, w, stride=st.down, padding=st.hl)[:, 0, :st.Tout]
            return out.reshape(B, C, -1) + x[..., :1]
        slow[name + "_torch"] = torch_form
        keep[name] = (x, y, st, kw, tab)
        fma, nbytes = B * C * st.Tout * st.Lp, 4 * B * C * (T + st.Tout)
        meta[name] = dict(spec=s["spec"], up=st.up, down=st.down, Tin=T, Tout=st.Tout, phase_len=st.Lp, fma=fma, bytes=nbytes,
                          lds_reads=2 * fma, lds_bytes_per_row=4 * (T + 2 * st.Lp + st.up * (st.Lp | 1)))
    Y = YARDSTICK
    xy = torch.randn(Y["B"], Y["C"], Y["T"], device=dev) * 30 + torch.empty(Y["B"], Y["C"], 1, device=dev).uniform_(-2e4, 2e4)
    pre = resolve(parse_eeg_preprocess(f"decimate={Y['decimate']},taps={Y['taps']}"), Y["C"], Y["T"], notice=None)
    taps = torch.as_tensor(pre.taps, dtype=torch.float32).to(dev)
    fns["yardstick_eeg_preprocess_decimate2_41taps"] = lambda: ops.eeg_preprocess(xy, taps, decimate=pre.q, edge=pre.edge)
    if which == "torch":
        return _windows(slow, warmup=1, window=2, rounds=3)
    res = dict(hbm_peak_bytes_per_s=HBM_PEAK, valu_f32_peak_flop_per_s=VALU_F32_PEAK, lds_b32_dwords_per_s=LDS_DWORDS_PER_S)
    res.update(_windows(fns))
    for name, m in meta.items():
        sec = res[name]["median_ms"] * 1e-3
        x, y, st, kw, tab = keep[name]
        m.update(share_of_f32_valu_peak=2 * m["fma"] / sec / VALU_F32_PEAK, share_of_hbm_peak=m["bytes"] / sec / HBM_PEAK,
                 share_of_lds_b32_rate=m["lds_reads"] / sec / LDS_DWORDS_PER_S,
                 two_calls_bitwise=bool(torch.equal(ops.eeg_resample(x, tab, **kw), y)))
        rows = y[:2, :3].cpu().numpy().astype(np.float64)                # six rows against the float64 rule, at the row's scale
        ref = resample_numpy(x[:2, :3].cpu().numpy(), st.tab, st.up, st.down, st.hl, st.edge)
        xs = x[:2, :3].double().cpu().numpy()
        m["max_err_over_centred_row_scale"] = float((np.abs(rows - ref) / np.abs(xs - xs[..., :1]).max(axis=-1, keepdims=True)).max())
        res[name].update(m)
    yard = res["yardstick_eeg_preprocess_decimate2_41taps"]["median_ms"]
    res["decimate_1_2_over_yardstick"] = res["decimate_1_2"]["median_ms"] / yard
    res["chisco_64_125_over_yardstick"] = res["chisco_64_125"]["median_ms"] / yard
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel", "torch"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eeg_resample.json"))
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a.step)))
        return
    res = dict(shapes=SHAPES, yardstick=dict(YARDSTICK, what="ops.eeg_preprocess, the FIR stage's decimation, timed in the same process; "
                                                           "expected ratio <= 2 from instruction counts, not a gate"))
    for which, limit in (("kernel", 240), ("torch", 240)):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", which], capture_output=True, text=True, timeout=limit)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            rc, err = r.returncode, r.stderr[-2000:]
        except subprocess.TimeoutExpired:
            line, rc, err = [], 124, f"no result within {limit} s"
        if rc != 0 or not line:
            res[which] = dict(failed=rc, stderr=err)
            print(which, "failed", rc, flush=True)
            if which == "kernel" or rc in (124, 134, 139, -6, -9, -11):
                break                                                     # nothing more on the device behind a fault or a hang
        else:
            res[which] = json.loads(line[-1][7:])
            print(which, json.dumps(res[which]), flush=True)
    if "median_ms" in res.get("torch", {}).get("chisco_64_125_torch", {}):
        for name in SHAPES:
            res[name + "_over_torch"] = res["kernel"][name]["median_ms"] / res["torch"][name + "_torch"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    if "failed" in res.get("kernel", {}):
        sys.exit(1)


if __name__ == "__main__":
    main()
