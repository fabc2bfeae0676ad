"""Rational resampling stage on the device: ign_eeg_resample_nct (ops.eeg_resample) against the float64 rule of
utils/eeg_resample.py at every place the kernel can go wrong (tests/eeg_resample_cases.py), then the stage inside the prefetcher
between the IIR and the FIR stages, and the harness."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from eeg_resample_cases import CASES, R, case
from eeg_spatial_cases import write_shards

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


def _run(ops, k, x, tab, **kw):
    return ops.eeg_resample(x, tab, up=k["up"], down=k["down"], half_len=k["hl"], edge=k["edge"], **kw)


def _probe_rows(B, C):
    """every row; for the CHISCO-sized case the first, the last and two in the middle"""
    every = [(b, c) for b in range(B) for c in range(C)]
    return every if len(every) <= 8 else [every[0], every[len(every) // 3], every[len(every) // 2], every[-1]]


# ------------------------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("label", list(CASES))
def test_kernel_is_the_float64_rule_repeatable_and_row_independent(label):
    """out - x[..., :1] against the float64 rule (fp32 input, fp32-rounded taps) minus the same pivot, each row at its own centred
    scale max_t |x - x[0]|, tol = 1e-4.  A priori: the final addition of the pivot rounds to half an ulp of |out| < 32768, 9.8e-4 uV,
    under 2e-5 of the >= 60 uV these rows span; the chain adds (Lp + 1) 2^-24 sum|tab||ue| < 4e-6 of the scale."""
    from conftest import parity
    dev, ops = _dev(), _ops()
    k = case(label)
    x, tab = _t(k["x"], dev), _t(k["tab"], dev)
    B, C, Tin = x.shape
    out = torch.full((B, C, k["Tout"]), float("nan"), device=dev)
    y = _run(ops, k, x, tab, out=out)
    assert y is out and y.dtype == torch.float32 and bool(torch.isfinite(y).all())            # every element was overwritten
    p = k["x"][..., :1].astype(np.float64)
    got = (y.cpu().numpy().astype(np.float64) - p) / k["scale"]
    want = (k["ref64"] - p) / k["scale"]
    e32 = float(np.abs((k["ref32"].astype(np.float64) - p) / k["scale"] - want).max())
    print(f"eeg_resample {label}: kernel {float(np.abs(got - want).max()):.3e} of the centred row scale from the float64 rule, "
          f"float32 numpy restatement {e32:.3e}; smallest row scale {float(k['scale'].min()):.1f}")
    parity(f"eeg_resample {label}", got, want, kind="scale", floor=1.0,
           ref_is="the float64 rule of utils/eeg_resample.py on the fp32 input and fp32 taps, pivot removed, per row over max|x - x[0]|")
    again = _run(ops, k, x, tab)
    assert again.data_ptr() != y.data_ptr() and torch.equal(again, y)
    for b, c in _probe_rows(B, C):
        alone = _run(ops, k, x[b:b + 1, c:c + 1].contiguous(), tab)
        assert alone.shape == (1, 1, k["Tout"]) and torch.equal(alone[0, 0], y[b, c]), (label, b, c)


@pytest.mark.parametrize("label", ["A_down_2_3", "B_up_3_2", "C_64_125_zero", "E_128_phases", "F_one_phase", "H_shortest_row"])
def test_constant_rows_come_back_bit_for_bit(label):
    dev, ops = _dev(), _ops()
    k = case(label)
    B, C, Tin = k["x"].shape
    p = k["x"][:, :, :1]                                               # every row's own offset, +-2e4 uV
    y = _run(ops, k, _t(np.broadcast_to(p, (B, C, Tin)), dev), _t(k["tab"], dev))
    assert np.array_equal(y.cpu().numpy(), np.broadcast_to(p, (B, C, k["Tout"])))


def test_a_non_contiguous_input_is_copied():
    dev, ops = _dev(), _ops()
    k = case("A_down_2_3")
    x, tab = _t(k["x"], dev), _t(k["tab"], dev)
    view = x.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    assert not view.is_contiguous() and torch.equal(_run(ops, k, view, tab), _run(ops, k, x, tab))


def test_refusals_raise_and_launch_nothing():
    dev, ops = _dev(), _ops()
    from ign_hip import _lib
    from ign_hip._lib import IgnError
    _lib.timing_enable(True)
    try:
        # one sample beyond the longest row, and one short of the shortest: `out` stays as it was
        k = case("I_longest_row")
        tab = _t(k["tab"], dev)
        out = torch.full((1, 1, 8131), 7.0, device=dev)
        with pytest.raises(IgnError, match="bytes of LDS"):
            _run(ops, k, torch.zeros(1, 1, 16262, device=dev), tab, out=out)
        k = case("H_shortest_row")
        tab = _t(k["tab"], dev)
        short = torch.full((1, 1, 21), 7.0, device=dev)
        with pytest.raises(IgnError, match="R=31"):
            _run(ops, k, torch.zeros(1, 1, 31, device=dev), tab, out=short)
        x = torch.zeros(1, 2, 50, device=dev)
        with pytest.raises(IgnError, match="lowest terms"):
            ops.eeg_resample(x, torch.zeros(4, 16, device=dev), up=4, down=6, half_len=30)
        with pytest.raises(IgnError, match=r"ceil\(\(2\*hl\+1\)/up\)"):
            ops.eeg_resample(x, tab, up=2, down=3, half_len=29)
        with pytest.raises(IgnError, match="does not hold up=3 phases"):
            ops.eeg_resample(x, tab, up=3, down=2, half_len=30)
        with pytest.raises(IgnError, match="not a positive ratio"):
            ops.eeg_resample(x, tab, up=2, down=0, half_len=30)
        with pytest.raises(IgnError, match="neither 'reflect' nor 'zero'"):
            ops.eeg_resample(x, tab, up=2, down=3, half_len=30, edge="odd")
        with pytest.raises(IgnError, match="float32"):
            ops.eeg_resample(x, tab.double(), up=2, down=3, half_len=30)
        with pytest.raises(IgnError, match="float32"):
            ops.eeg_resample(x.double(), tab, up=2, down=3, half_len=30)
        with pytest.raises(IgnError, match="runs on the MI355X only"):
            ops.eeg_resample(x, tab.cpu(), up=2, down=3, half_len=30)
        with pytest.raises(IgnError, match="out must be"):
            ops.eeg_resample(x, tab, up=2, down=3, half_len=30, out=torch.zeros(1, 2, 33, device=dev))
        with pytest.raises(IgnError, match="expected x"):
            ops.eeg_resample(x[0], tab, up=2, down=3, half_len=30)
        torch.cuda.synchronize()
        assert _lib.timing_read("eeg_resample")[1] == 0                 # nothing was launched
        assert bool((out == 7.0).all()) and bool((short == 7.0).all())
        assert tuple(ops.eeg_resample(x, tab, up=2, down=3, half_len=30).shape) == (1, 2, 34)
        torch.cuda.synchronize()
        assert _lib.timing_read("eeg_resample")[1] == 1
    finally:
        _lib.timing_enable(False)


# --------------------------------------------------------------------------------------------------------- prefetcher, harness
def _ns(root, **kw):
    from argparse import Namespace
    base = dict(task_name="classification", data="EEG", root_path=str(root), batch_size=8, num_workers=0, seed=0,
                device_standardise=True)
    base.update(kw)
    return Namespace(**base)


@pytest.mark.parametrize("flag", ["train", "test"])
def test_chain_iir_resample_preprocess_is_the_three_ops_composed_by_hand(tmp_path, flag):
    dev, ops = _dev(), _ops()
    from data_provider.data_factory import data_provider
    from exp.experiment_classification import Experiment
    write_shards(str(tmp_path), T=400)
    ds, loader = data_provider(_ns(tmp_path, eeg_iir="hp=1,notch=50", eeg_resample="rate=256", eeg_preprocess="band=8:30,sfreq=256"), flag)
    rs, pre, iir = ds.resample, ds.pre, ds.iir
    assert (rs.Tin, rs.Tout, ds.seq_len, ds.enc_in) == (400, 205, 205, 6) and len(pre.taps) == 107 and iir.pad == 21
    torch.manual_seed(11)
    raw = [(x.clone(), y.clone()) for x, y, _ in loader]                # the loader's own order under this seed
    torch.manual_seed(11)
    got = list(Experiment._prefetch(SimpleNamespace(device=dev), loader))
    assert len(got) == len(raw) == -(-len(ds) // 8)
    coef, tab = _t(iir.table, dev), _t(rs.tab, dev)
    taps = torch.as_tensor(pre.taps, dtype=torch.float32).to(dev)
    for (a, b, m), (x, y) in zip(got, raw):
        v = ops.eeg_iir(x.to(dev), coef, pad=iir.pad, g0=iir.g0)
        v = ops.eeg_resample(v, tab, up=64, down=125, half_len=rs.hl, edge="reflect")
        want, mask = ops.eeg_preprocess(v, taps, decimate=pre.q, edge=pre.edge, channels=pre.Cout, timepoints=pre.Tout)
        assert a.is_cuda and tuple(a.shape) == (x.shape[0], 205, 6) and torch.equal(a, want) and torch.equal(m, mask)
        assert torch.equal(b.cpu(), y) and bool(torch.isfinite(a).all())


def test_harness_trains_two_steps_on_resampled_rows_and_records_the_stage(tmp_path, monkeypatch):
    _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    import run as driver
    from exp.experiment_classification import Experiment
    m = R()
    write_shards(str(tmp_path), T=125)
    monkeypatch.chdir(tmp_path)
    args = driver.get_args(["--model", "SBM", "--data", "EEG3", "--data_root", str(tmp_path), "--dataset", "chisco_npy",
                            "--train_epochs", "1", "--batch_size", "9", "--seed", "0", "--num_workers", "0",
                            "--eeg_resample", "rate=256"])
    driver.set_seed(0)
    exp = Experiment(args)
    assert args.enc_in == 6 and args.seq_len == 64 == exp.train_data.resample.Tout       # the model is built for Tout time steps
    assert exp.val_data.resample.Tout == 64 and exp.test_data.seq_len == 64
    per_step, step = exp.train_one_epoch(0, 0)
    losses = [float(v) for v in per_step]
    assert step == 2 == len(losses) and all(np.isfinite(v) for v in losses), losses
    rec = json.load(open(os.path.join(exp.checkpoint_dir, m.FILE_NAME)))
    assert m.parse_eeg_resample(rec["spec"]) == exp.train_data.resample.spec
    assert (rec["sfreq_in"], rec["sfreq_out"], rec["up"], rec["down"], rec["half"], rec["beta"], rec["edge"], rec["Tin"], rec["Tout"]) == (
        500.0, 256.0, 64, 125, 10, 5.0, "reflect", 125, 64)


def test_a_run_without_the_flag_never_launches_the_kernel(tmp_path):
    dev = _dev()
    _ops()
    from data_provider.data_factory import data_provider
    from exp.experiment_classification import Experiment
    from ign_hip import _lib
    write_shards(str(tmp_path))
    me = SimpleNamespace(device=dev)
    _lib.timing_enable(True)
    try:
        for kw in ({}, dict(eeg_resample="none"), dict(eeg_resample="rate=500")):
            _, loader = data_provider(_ns(tmp_path, **kw), "test")
            plain = list(Experiment._prefetch(me, loader))
        torch.cuda.synchronize()
        assert _lib.timing_read("eeg_resample")[1] == 0
        _, loader = data_provider(_ns(tmp_path, eeg_resample="rate=256"), "test")
        on = list(Experiment._prefetch(me, loader))
        torch.cuda.synchronize()
        assert _lib.timing_read("eeg_resample")[1] == len(on) == len(plain) == 1
    finally:
        _lib.timing_enable(False)
    assert tuple(plain[0][0].shape) == (4, 64, 6) and tuple(on[0][0].shape) == (4, 33, 6)
