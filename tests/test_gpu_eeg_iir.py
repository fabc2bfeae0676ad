"""Zero-phase IIR stage on the device: ign_eeg_iir_nct (ops.eeg_iir) against the float64 rule of utils/eeg_iir.py at every place
the kernel can go wrong (tests/eeg_iir_cases.py), then the stage inside the prefetcher, the alignment fit and the harness."""
import json
import os

import numpy as np
import pytest
import torch

from eeg_iir_cases import CASES, I, case, check_rows
from eeg_spatial_cases import S, write_shards

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ops():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    return ops


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(ops, k, x, dev, **kw):
    return ops.eeg_iir(x, _t(k["table"], dev), pad=k["pad"], g0=k["g0"], **kw)


# ------------------------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("label", list(CASES))
def test_kernel_is_the_float64_rule_repeatable_and_row_independent(label):
    from conftest import parity
    dev, ops = _dev(), _ops()
    k = case(label)
    x = _t(k["x"], dev)
    B, C, T = x.shape
    out = torch.full((B, C, T), float("nan"), device=dev)
    y = _run(ops, k, x, dev, out=out)
    assert y is out and y.dtype == torch.float32 and bool(torch.isfinite(y).all())            # every element was overwritten
    check_rows(label, y.cpu().numpy(), k["ref64"], k["scale"])
    # the ledger: the same comparison at the scale of what the rows carry (the larger of the result and the signal)
    parity(f"eeg_iir {label}", y, k["ref64"].astype(np.float32), kind="scale", floor=float(k["scale"].max()), f64=k["ref64"],
           ref_is="the float64 rule of utils/eeg_iir.py rounded to fp32 once")
    again = _run(ops, k, x, dev)
    assert again.data_ptr() != y.data_ptr() and torch.equal(again, y)
    for b in range(B):
        for c in range(C):
            alone = _run(ops, k, x[b:b + 1, c:c + 1].contiguous(), dev)
            assert alone.shape == (1, 1, T) and torch.equal(alone[0, 0], y[b, c]), (label, b, c)


@pytest.mark.parametrize("label", list(CASES))
def test_constant_rows_give_g0_times_the_constant_exactly(label):
    dev, ops = _dev(), _ops()
    k = case(label)
    B, C, T = k["x"].shape
    p = k["x"][:, :, :1]                                               # every row's own offset, +-2e4 uV
    y = _run(ops, k, _t(np.broadcast_to(p, (B, C, T)), dev), dev)
    want = (k["g0"] * np.broadcast_to(p, (B, C, T)).astype(np.float64)).astype(np.float32)
    assert np.array_equal(y.cpu().numpy(), want)


def test_a_non_contiguous_input_is_copied():
    dev, ops = _dev(), _ops()
    k = case("F_full_chain")
    x = _t(k["x"], dev)
    view = x.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    assert not view.is_contiguous() and torch.equal(_run(ops, k, view, dev), _run(ops, k, x, dev))


def test_one_sample_beyond_the_longest_row_is_too_big_and_other_refusals():
    dev, ops = _dev(), _ops()
    from ign_hip._lib import IgnError
    k = case("J_longest_row")
    T = k["x"].shape[-1]
    x = torch.zeros(1, 1, T + 1, device=dev)
    out = torch.full((1, 1, T + 1), 7.0, device=dev)
    with pytest.raises(IgnError, match="8193"):
        _run(ops, k, x, dev, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                    # nothing was launched
    small = torch.zeros(1, 2, 9, device=dev)
    with pytest.raises(IgnError, match="P=9"):
        _run(ops, k, small, dev)
    with pytest.raises(IgnError, match="coef must be a float64"):
        ops.eeg_iir(small, _t(k["table"], dev).float(), pad=3, g0=1.0)
    with pytest.raises(IgnError, match="coef must be a float64"):
        ops.eeg_iir(small, _t(k["table"], dev)[:, :6], pad=3, g0=1.0)
    with pytest.raises(IgnError, match="coef must be a float64"):
        ops.eeg_iir(small, torch.from_numpy(k["table"].copy()), pad=3, g0=1.0)
    with pytest.raises(IgnError, match="out must be"):
        ops.eeg_iir(small, _t(k["table"], dev), pad=3, g0=1.0, out=torch.zeros(1, 2, 8, device=dev))
    with pytest.raises(IgnError, match="expected x"):
        ops.eeg_iir(small[0], _t(k["table"], dev), pad=3, g0=1.0)
    with pytest.raises(IgnError, match="float32"):
        ops.eeg_iir(small.double(), _t(k["table"], dev), pad=3, g0=1.0)


# ------------------------------------------------------------------------------------------------- prefetcher, fit, harness
IIR = "hp=1,notch=50"


@pytest.mark.parametrize("pre", [None, "band=8:30,taps=41"], ids=["standardise", "bandpass"])
def test_prefetcher_spatial_iir_preprocess_equals_the_cpu_item_path(tmp_path, pre):
    """The raw device path (spatial launch, IIR launch, then the standardisation or the band-pass transform) against the CPU item
    path (the spatial rule's fp32 restatement, the float64 IIR rule rounded to fp32 once, then the numpy rules): conftest.parity,
    element-wise at the project's tolerance, with the float64 form of the whole path beside it.  The high-pass takes the recording's
    offset out in float64, so what the later fp32 stages see is at the signal's own scale."""
    from conftest import parity
    dev, s, m = _dev(), S(), I()
    _ops()
    from data_provider.device_prefetch import DevicePrefetcher
    from data_provider.eeg_chain import EEGChain
    from data_provider.eeg_npy import EEGNpyDataset, collate_raw_group, per_sample_standardise
    from data_provider.uea import collate_fn
    from utils.eeg_filter import filterbank_numpy, pad_time
    X, y, subj = write_shards(str(tmp_path))
    kw = dict(chain=EEGChain(spatial="ref=car", iir=IIR, preprocess=pre))
    cpu = EEGNpyDataset(str(tmp_path), flag="train", **kw)
    raw = EEGNpyDataset(str(tmp_path), flag="train", raw=True, **kw)
    assert raw.iir.pad == 21 and raw.iir.ns == 3 and (raw.enc_in, raw.seq_len) == (cpu.enc_in, cpu.seq_len) == (6, 64)
    W = raw.spatial.W
    want = list(torch.utils.data.DataLoader(cpu, batch_size=8, shuffle=False, collate_fn=lambda b: collate_fn(b, max_len=cpu.seq_len)))
    loader = torch.utils.data.DataLoader(raw, batch_size=8, shuffle=False, collate_fn=collate_raw_group, pin_memory=True)
    assert raw.chain.names == ["spatial", "iir"] + ([] if pre is None else ["preprocess"])
    got = list(DevicePrefetcher(loader, dev, transform=raw.chain.device_transform(dev)))
    assert len(got) == len(want) == 3
    for i, ((a, b, ma), (c, d, n)) in enumerate(zip(got, want)):
        j = raw.idx[8 * i:8 * i + 8]
        v64 = m.iir_numpy(s.spatial_numpy(X[j], W, raw.group[j]), raw.iir.table, raw.iir.pad, raw.iir.g0)
        if pre is None:
            f64 = np.swapaxes(per_sample_standardise(v64), 1, 2)
        else:
            p = raw.pre
            f64, _ = pad_time(filterbank_numpy(v64, p.taps2d.astype(np.float32), None, p.q, p.edge, p.Cout, p.Tout), p.Tout)
        assert a.is_cuda and a.shape == c.shape == f64.shape == (len(j), 64, 6)
        e_ref = float((np.abs(c.double().numpy() - f64) / (1.0 + np.abs(f64))).max())
        e_hip = float((np.abs(a.double().cpu().numpy() - f64) / (1.0 + np.abs(f64))).max())
        print(f"eeg_iir prefetcher {pre} batch {i}: CPU item path vs float64 {e_ref:.3e}, device path vs float64 {e_hip:.3e}")
        parity(f"eeg_iir prefetcher {pre} batch {i}", a, c, kind="elem", f64=f64,
               ref_is="CPU item path: fp32 restatement of the spatial rule, the float64 IIR rule rounded once, then the numpy rules")
        assert torch.equal(b.cpu(), d) and torch.equal(ma.cpu().bool(), n.bool())


def test_harness_trains_with_the_stage_fits_the_alignment_behind_it_and_records_it(tmp_path, monkeypatch):
    """Experiment under --eeg_spatial ref=car,align=euclid --eeg_iir hp=1,notch=50: the alignment is fitted on the device on the
    FILTERED rows (it differs from the fit without the stage and equals the host float64 fit on filtered rows to the 1e-5 max|W|
    of tests/test_gpu_eeg_spatial.py), one epoch gives finite losses, eeg_iir.json is written."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    import run as driver
    from exp.experiment_classification import Experiment
    s, m = S(), I()
    write_shards(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    args = driver.get_args(["--model", "SBM", "--data", "EEG3", "--data_root", str(tmp_path), "--dataset", "chisco_npy",
                            "--train_epochs", "1", "--batch_size", "8", "--seed", "0", "--num_workers", "0",
                            "--eeg_spatial", "ref=car,align=euclid", "--eeg_iir", IIR])
    driver.set_seed(0)
    exp = Experiment(args)
    assert args.enc_in == 6 and args.seq_len == 64                          # the stage keeps the shape
    st, iir = exp.train_data.spatial, exp.train_data.iir
    assert st.fitted and iir.pad == 21 and exp.val_data.iir.pad == 21
    per_step, step = exp.train_one_epoch(0, 0)
    losses = [float(v) for v in per_step]
    assert step == 3 == len(losses) and all(np.isfinite(v) for v in losses), losses
    rec = json.load(open(os.path.join(exp.checkpoint_dir, m.FILE_NAME)))
    assert m.parse_eeg_iir(rec["spec"]) == iir.spec and rec["pad"] == 21 and np.array_equal(np.asarray(rec["table"]), iir.table)
    batches = list(exp.train_data.raw_batches(8))
    host = s.fit_alignment(batches, st.W0, 3, 1e-6, notice=None, post=exp.train_data.chain.alignment_post(dev))              # numpy float64 on filtered rows
    plain = s.fit_alignment(batches, st.W0, 3, 1e-6, notice=None)
    d_host = float(np.abs(st.W - host).max()) / float(np.abs(host).max())
    d_plain = float(np.abs(st.W - plain).max()) / float(np.abs(plain).max())
    print(f"eeg_iir alignment: device fit vs host fit on filtered rows {d_host:.3e}, vs the fit without the stage {d_plain:.3e}")
    assert d_host <= 1e-5 and d_plain > 1e-2
    on_dev = [(torch.from_numpy(x).to(dev), None, torch.from_numpy(g).to(dev)) for x, _, g in batches]
    assert s.fit_alignment(on_dev, st.W0, 3, 1e-6, notice=None, post=exp.train_data.chain.alignment_post(dev)).tobytes() == st.W.tobytes()
