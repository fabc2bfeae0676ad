"""Artifact stage on the device: ign_eeg_artifact_stats_nct + ign_eeg_artifact_apply_nct (ops.eeg_artifact) against the numpy rule of
utils/eeg_artifact.py at every place the kernels can go wrong (tests/eeg_artifact_cases.py) -- statistics, verdicts and good rows
bit for bit, repaired rows against the float64 repair within the a-priori bound -- then the stage inside the prefetcher in front of
the spatial and IIR stages, the report pass, and the harness."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from eeg_artifact_cases import A, CASES, KEYS, RUNS, expected, plant
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
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _filled(B, C, T, dev):
    return (torch.full((B, C, T), float("nan"), device=dev), torch.full((B, C), 255, dtype=torch.uint8, device=dev),
            torch.full((B, C, 2), float("nan"), device=dev))


def _check_against_rule(label, k, y, verdict, stats):
    """statistics and verdicts exactly, good rows to the bit, repaired rows inside the a-priori bound and the project's budget"""
    from conftest import parity
    y, verdict, stats = y.cpu().numpy(), verdict.cpu().numpy(), stats.cpu().numpy()
    assert np.array_equal(stats, k["stats"]), label
    assert np.array_equal(verdict, k["verdict"]), label
    rep = (k["verdict"] >= 1) & (k["verdict"] <= 3)
    assert y[~rep].tobytes() == k["y32"][~rep].tobytes(), label
    if not rep.any():
        return
    assert np.isfinite(y[rep]).all()
    err = np.abs(y.astype(np.float64) - k["y64"])
    e32 = np.abs(k["y32"].astype(np.float64) - k["y64"])
    ratio = float((err[rep] / np.maximum(k["bound"][rep], 1e-300)).max())
    for b in np.flatnonzero(rep.any(1)):
        print(f"eeg_artifact {label} sample {b}: kernel {err[b][rep[b]].max() / k['scale'][b]:.3e} of the good rows' centred scale "
              f"{k['scale'][b]:.1f} from the float64 repair, float32 numpy restatement {e32[b][rep[b]].max() / k['scale'][b]:.3e}; "
              f"worst error / a-priori bound {ratio:.4f}")
        parity(f"eeg_artifact {label} sample {b}", y[b][rep[b]] / k["scale"][b], k["y64"][b][rep[b]] / k["scale"][b], kind="scale",
               floor=1.0, ref_is="the float64 repair of utils/eeg_artifact.py on the fp32 inputs, over the good rows' largest centred amplitude")
    assert (err[rep] <= k["bound"][rep]).all(), (label, ratio)


def _probe_samples(B):
    return range(B) if B <= 5 else (0, B - 1)


def _probe_rows(B, C):
    every = [(b, c) for b in range(B) for c in range(C)]
    return every if len(every) <= 8 else [every[0], every[len(every) // 3], every[len(every) // 2], every[-1]]


# ------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("label,variant", RUNS, ids=[f"{a}-{b}" for a, b in RUNS])
def test_kernels_are_the_rule_overwrite_everything_and_repeat(label, variant):
    dev, ops = _dev(), _ops()
    k = expected(label, variant)
    x, w = _t(k["x"], dev), _t(k["w"], dev)
    B, C, T = x.shape
    bufs = _filled(B, C, T, dev)
    y, verdict, stats = ops.eeg_artifact(x, neighbors=w, out=bufs, **k["keys"])
    assert y is bufs[0] and verdict is bufs[1] and stats is bufs[2]
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(stats).all()) and int(verdict.max()) <= 4     # all overwritten
    _check_against_rule(f"{label} {variant}", k, y, verdict, stats)
    again = ops.eeg_artifact(x, neighbors=w, **k["keys"])
    assert again[0].data_ptr() != y.data_ptr() and all(torch.equal(p, q) for p, q in zip(again, (y, verdict, stats)))


@pytest.mark.parametrize("label", list(CASES))
def test_a_sample_alone_gives_its_bits_and_a_row_alone_its_statistics(label):
    dev, ops = _dev(), _ops()
    k = expected(label, CASES[label][1][0])
    x, w = _t(k["x"], dev), _t(k["w"], dev)
    B, C, T = x.shape
    y, verdict, stats = ops.eeg_artifact(x, neighbors=w, **k["keys"])
    for b in _probe_samples(B):
        alone = ops.eeg_artifact(x[b:b + 1].contiguous(), neighbors=w, **k["keys"])
        assert all(torch.equal(p[0], q[b]) for p, q in zip(alone, (y, verdict, stats))), (label, b)
    for b, c in _probe_rows(B, C):
        row = ops.eeg_artifact(x[b:b + 1, c:c + 1].contiguous(), **k["keys"])[2]
        assert row.shape == (1, 1, 2) and torch.equal(row[0, 0], stats[b, c]), (label, b, c)


def test_without_clip_and_without_a_bad_electrode_out_is_the_input():
    dev, ops = _dev(), _ops()
    for label in ("B_65", "D_2049"):
        x = _t(expected(label, "all")["x"], dev)
        y, verdict, _ = ops.eeg_artifact(x, flat=0.01, noisy=8.0)
        assert not bool(verdict.any()) and y.data_ptr() != x.data_ptr() and y.cpu().numpy().tobytes() == x.cpu().numpy().tobytes()


def test_a_non_contiguous_input_is_copied_and_wide_channel_counts_take_narrower_tiles():
    dev, ops = _dev(), _ops()
    k = expected("H_verdicts_C7", "all")
    x = _t(k["x"], dev)
    view = x.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    assert not view.is_contiguous() and all(torch.equal(p, q) for p, q in zip(ops.eeg_artifact(view, **k["keys"]), ops.eeg_artifact(x, **k["keys"])))
    m = A()
    rng = np.random.RandomState(9)
    for C in (257, 600):                                                 # tiles of 32 and of 16 samples
        xs = (rng.randn(1, C, 70) * 20.0 + rng.uniform(-2e4, 2e4, size=(1, C, 1))).astype(np.float32)
        xs[0, 5] = xs[0, 5, 0]
        xs[0, C - 1, 69] = np.nan
        want = m.artifact_numpy(xs, repair64=True, **KEYS["all"])
        y, verdict, stats = ops.eeg_artifact(_t(xs, dev), **KEYS["all"])
        assert np.array_equal(verdict.cpu().numpy(), want[1]) and np.array_equal(stats.cpu().numpy(), want[2])
        rep = want[1] != 0
        assert rep.sum() == 2 and np.array_equal(y.cpu().numpy()[~rep].astype(np.float64), want[0][~rep])
        good = ~rep[0]
        scale = np.abs(want[0][0, good] - want[2][0, good, 0:1].astype(np.float64)).mean(0)       # all-ones weights: the bound's sum
        assert (np.abs(y.cpu().numpy()[rep] - want[0][rep]) <= (good.sum() + 3) * 2.0 ** -24 * scale).all()


def test_refusals_raise_and_launch_nothing():
    dev, ops = _dev(), _ops()
    from ign_hip import _lib
    from ign_hip._lib import IgnError
    _lib.timing_enable(True)
    try:
        x = torch.zeros(1, 2, 50, device=dev)
        with pytest.raises(IgnError, match="T=16385"):
            ops.eeg_artifact(torch.zeros(1, 1, 16385, device=dev), clip=6.0)
        with pytest.raises(IgnError, match="C=1025"):
            ops.eeg_artifact(torch.zeros(1, 1025, 4, device=dev), clip=6.0)
        with pytest.raises(IgnError, match="negative or non-finite"):
            ops.eeg_artifact(x, neighbors=torch.tensor([[0.0, -1.0], [1.0, 0.0]], device=dev))
        with pytest.raises(IgnError, match="negative or non-finite"):
            ops.eeg_artifact(x, neighbors=torch.tensor([[0.0, float("nan")], [1.0, 0.0]], device=dev))
        with pytest.raises(IgnError, match="neighbors must be"):
            ops.eeg_artifact(x, neighbors=torch.ones(3, 3, device=dev))
        with pytest.raises(IgnError, match="neighbors must be"):
            ops.eeg_artifact(x, neighbors=torch.ones(2, 2))
        with pytest.raises(IgnError, match="float32"):
            ops.eeg_artifact(x.double())
        with pytest.raises(IgnError, match="out must be"):
            ops.eeg_artifact(x, out=torch.zeros(1, 2, 49, device=dev))
        with pytest.raises(IgnError, match="expected x"):
            ops.eeg_artifact(x[0])
        torch.cuda.synchronize()
        assert _lib.timing_read("eeg_artifact_stats")[1] == 0 and _lib.timing_read("eeg_artifact_apply")[1] == 0     # nothing was launched
        assert int(ops.eeg_artifact(x, clip=6.0)[1].sum()) == 0
        torch.cuda.synchronize()
        assert _lib.timing_read("eeg_artifact_stats")[1] == 1 and _lib.timing_read("eeg_artifact_apply")[1] == 1
    finally:
        _lib.timing_enable(False)


# --------------------------------------------------------------------------------------------------------- prefetcher, harness
FLAG = "clip=6,flat=0.01,noisy=8"


def _ns(root, **kw):
    from argparse import Namespace
    base = dict(task_name="classification", data="EEG", root_path=str(root), batch_size=8, num_workers=0, seed=0,
                device_standardise=True)
    base.update(kw)
    return Namespace(**base)


def _planted(root, T=100):
    X, _, _ = write_shards(str(root), T=T)
    planted = plant(X)
    np.save(os.path.join(str(root), "X.npy"), X)
    return X, planted


def test_prefetcher_repairs_in_front_of_car_and_iir_and_without_the_stage_the_batches_hold_nan(tmp_path):
    from conftest import parity
    dev, ops = _dev(), _ops()
    from data_provider.data_factory import data_provider
    from exp.experiment_classification import Experiment
    m = A()
    X, planted = _planted(tmp_path)
    on = dict(eeg_artifact=FLAG, eeg_spatial="ref=car", eeg_iir="hp=1")
    ds, loader = data_provider(_ns(tmp_path, **on), "train")
    assert ds.chain.names == ["artifact", "spatial", "iir"] and loader.eeg_chain is ds.chain
    torch.manual_seed(11)
    raw = [x.clone() for x, _, _ in loader]
    torch.manual_seed(11)
    got = list(Experiment._prefetch(SimpleNamespace(device=dev), loader))
    cpu_ds, _ = data_provider(_ns(tmp_path, device_standardise=False, **on), "train")
    items = {cpu_ds.idx[i]: cpu_ds[i][0].numpy() for i in range(len(cpu_ds))}
    W, coef = _t(ds.spatial.W, dev), _t(ds.iir.table, dev)
    worst = 0.0
    for (a, _, mask), x in zip(got, raw):
        # the stage's own output on the loader's raw batch: the rule, exact outside the repaired rows
        y, verdict, stats = ops.eeg_artifact(x.to(dev), clip=6.0, flat=0.01, noisy=8.0)
        want = m.artifact_numpy(x.numpy(), repair64=True, clip=6.0, flat=0.01, noisy=8.0)
        assert np.array_equal(verdict.cpu().numpy(), want[1]) and np.array_equal(stats.cpu().numpy(), want[2])
        rep = (want[1] >= 1) & (want[1] <= 3)
        assert rep.any(1).all() and np.array_equal(y.cpu().numpy()[~rep].astype(np.float64), want[0][~rep])
        # the batch is the device ops composed by hand, to the bit, and finite everywhere
        v = ops.eeg_iir(ops.eeg_spatial(y, W), coef, pad=ds.iir.pad, g0=ds.iir.g0)
        assert torch.equal(a, ops.standardise_nct_to_btc(v)) and bool(torch.isfinite(a).all()) and bool(mask.all())
        # and the CPU item path of the same trials, at the project's budget
        for i in range(x.shape[0]):
            j = int(np.flatnonzero((X == x[i].numpy()).reshape(len(X), -1).sum(1) >= X[0].size - 1)[0])      # the NaN is equal to nothing
            rec = parity(f"eeg_artifact prefetcher trial {j}", a[i].cpu().numpy(), items[j], kind="elem",
                         ref_is="the CPU item path: the numpy rules of the three stages and the standardisation")
            worst = max(worst, rec["err_over_1e4"])
    print(f"eeg_artifact prefetcher: worst distance from the CPU item path {worst:.3f} of the 1e-4 budget")
    # the same run without the stage: the NaN reaches the model's input through the common average reference
    ds, loader = data_provider(_ns(tmp_path, eeg_spatial="ref=car", eeg_iir="hp=1"), "train")
    if planted["nan"][0] in ds.idx:
        plain = torch.cat([b[0] for b in Experiment._prefetch(SimpleNamespace(device=dev), loader)])
        assert not bool(torch.isfinite(plain).all())
        assert int((~torch.isfinite(plain)).flatten(1).any(1).sum()) == 1 and bool((~torch.isfinite(plain)).flatten(1).all(1).any())


def test_report_pass_counts_what_was_planted(tmp_path):
    dev = _dev()
    _ops()
    from data_provider.data_factory import data_provider, ordered_loader
    from data_provider.device_prefetch import DevicePrefetcher
    X, planted = _planted(tmp_path)
    ds, loader = data_provider(_ns(tmp_path, eeg_artifact=FLAG + ",report"), "train")
    rep = ds.artifact.report_pass(DevicePrefetcher(ordered_loader(loader), dev))
    idx = list(ds.idx)
    n = len(idx)
    want = A().resolve_artifact(FLAG, 6, 100).report_pass([(X[idx], None, None)])        # the numpy rule on the same trials
    assert rep == want and rep["trials"] == n == rep["repaired_trials"]
    assert rep["flat"] == [0, n, 0, 0, 0, 0] and rep["unrepaired"] == [0] * 6
    assert rep["noisy"] == [0, 0, 0, 0, sum(i in idx for i in planted["noisy_trials"]), 0]
    assert rep["nonfinite"] == [0, 0, int(planted["nan"][0] in idx), 0, 0, 0]


def test_harness_trains_two_steps_behind_the_stage_and_writes_the_record(tmp_path, monkeypatch, capsys):
    _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    import run as driver
    from exp.experiment_classification import Experiment
    m = A()
    _planted(tmp_path, T=64)
    monkeypatch.chdir(tmp_path)
    args = driver.get_args(["--model", "SBM", "--data", "EEG3", "--data_root", str(tmp_path), "--dataset", "chisco_npy",
                            "--train_epochs", "1", "--batch_size", "9", "--seed", "0", "--num_workers", "0",
                            "--eeg_artifact", FLAG + ",report", "--eeg_spatial", "ref=car,align=euclid", "--eeg_iir", "hp=1"])
    driver.set_seed(0)
    exp = Experiment(args)
    assert args.enc_in == 6 and args.seq_len == 64 and exp.train_data.chain.names == ["artifact", "spatial", "iir"]
    assert exp.train_data.spatial.fitted and np.isfinite(exp.train_data.spatial.W).all()      # fitted on repaired rows: no NaN in the Grams
    per_step, step = exp.train_one_epoch(0, 0)
    losses = [float(v) for v in per_step]
    assert step == 2 == len(losses) and all(np.isfinite(v) for v in losses), losses
    rec = json.load(open(os.path.join(exp.checkpoint_dir, m.FILE_NAME)))
    assert m.parse_eeg_artifact(rec["spec"]) == exp.train_data.artifact.spec and rec["weights"] is None
    n = len(exp.train_data)
    assert rec["report"]["trials"] == n and rec["report"]["flat"][1] == n and rec["report"] == exp.train_data.artifact.report
    assert f"eeg_artifact: {n} training trials, {n} (100.0%) with a repaired electrode" in capsys.readouterr().out
