"""CPU tests of the regression task (--task_name regression): the .ts target parser, Monashloader against the reference's
loader, the one-stride subsampling rule (repair R2), the C ABI rows of the CRPS tail, the torch CRPSLoss against the
reference's, and the regression harness end to end with the CPU oracle models."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden

import speech_imagery_eeg_amd  # noqa: F401  (puts the package directory on sys.path)

TS = os.path.join(GOLDEN, "ts")


# ----------------------------------------------------------------------------------------------- .ts reader
def test_load_ts_reads_float_targets(tmp_path):
    from data_provider.ts_reader import load_ts, write_ts
    rng = np.random.RandomState(0)
    X = [rng.randn(2, 9) for _ in range(4)]
    y = [1.5, -2.25, 1e-3, 7.0]
    p = str(tmp_path / "R_TRAIN.ts")
    write_ts(p, X, y, regression=True)
    cases, labels, meta = load_ts(p)
    assert labels == y and all(isinstance(v, float) for v in labels)
    assert len(cases) == 4 and np.array_equal(cases[1][0], np.asarray([float(repr(float(v))) for v in X[1][0]]))
    cases, labels, _ = load_ts(os.path.join(TS, "RegEq_TRAIN.ts"))
    assert len(labels) == 9 and all(isinstance(v, float) for v in labels) and len(cases[0]) == 2


def test_load_ts_classification_unchanged():
    """The committed UEA fixtures carry @classLabel AND @targetlabel: class labels win, as strings."""
    from data_provider.ts_reader import load_ts
    for name in ("EqLen_TRAIN.ts", "Missing_TRAIN.ts", "Ragged_TRAIN.ts"):
        cases, labels, meta = load_ts(os.path.join(TS, name))
        assert all(isinstance(v, str) for v in labels) and set(labels) <= {"0", "1", "2"}
        assert len(cases[0]) == 3


# ----------------------------------------------------------------------------------------------- Monashloader
@pytest.mark.parametrize("stem", ["RegEq_TRAIN", "RegEq_TEST", "RegRagged_TRAIN", "RegMissing_TRAIN"])
def test_monashloader_matches_reference(stem):
    from data_provider.data_loader import Monashloader
    g = golden("monash_contract")
    edges = g["RegEq_TRAIN_edges"] if stem == "RegEq_TEST" else None
    ds = Monashloader(TS, bin_edges=edges, file_list=[stem + ".ts"])
    np.testing.assert_array_equal(ds.bin_edges, g[f"{stem}_edges"])
    assert ds.bin_edges.dtype == np.float64 and np.isposinf(ds.bin_edges[-1]) and len(ds.bin_edges) == 10
    assert ds.num_classes == 10 and len(ds.class_names) == 10
    assert ds.max_seq_len == int(g[f"{stem}_maxlen"])
    np.testing.assert_allclose(ds.feature_df, g[f"{stem}_feature"], rtol=1e-12, atol=1e-12)
    assert ds.labels_df.dtype == np.float32 and ds.labels_df.shape == g[f"{stem}_target"].shape
    np.testing.assert_array_equal(ds.labels_df, g[f"{stem}_target"].astype(np.float32))
    x, t = ds[1]
    idx = g[f"{stem}_index"]
    np.testing.assert_allclose(x.numpy(), g[f"{stem}_feature"][idx == 1], rtol=1e-12, atol=1e-12)
    assert t.dtype == torch.float32 and t.shape == (1,)


def test_monash_val_and_test_take_the_train_edges(tmp_path):
    import run
    from data_provider.data_factory import data_provider
    d = tmp_path / "Reg"
    d.mkdir()
    for split in ("TRAIN", "TEST"):
        os.symlink(os.path.join(TS, f"RegEq_{split}.ts"), str(d / f"RegEq_{split}.ts"))
    a = run.get_args(["--task_name", "regression", "--data", "Monash", "--data_root", str(tmp_path), "--dataset", "Reg",
                      "--batch_size", "4"])
    tr, _ = data_provider(a, "train")
    te, loader = data_provider(a, "test", bin_edges=tr.bin_edges)
    assert np.array_equal(te.bin_edges, tr.bin_edges)
    own = np.linspace(te.labels_df.min(), te.labels_df.max(), 11)[1:-1]
    assert not np.allclose(te.bin_edges[:-1], own)               # not the test split's own range
    X, y, m = next(iter(loader))
    assert X.shape == (4, 24, 2) and y.dtype == torch.float32 and m.shape == (4, 24)


# ----------------------------------------------------------------------------------------------- R2 subsampling
def test_subsample_stride_rule():
    from data_provider.uea import subsample_stride
    assert [subsample_stride(T) for T in (10, 999, 1000, 1001, 1500, 2000, 2001, 17984)] == [1, 1, 1, 2, 2, 2, 3, 18]


def test_collate_subsampled_every_batch_uses_one_stride():
    """T = 1500: every batch is padded to 1500 samples and takes every second one -- not the first 750 (the reference's
    second and later batches are clipped to the first batch's subsampled length)."""
    from data_provider.uea import collate_subsampled, subsample_stride
    T = 1500
    s = subsample_stride(T)
    items = [(torch.arange(L * 2, dtype=torch.float64).reshape(L, 2), torch.tensor([0.5], dtype=torch.float32))
             for L in (1500, 1203, 640)]
    X, y, mask = collate_subsampled(items, max_len=T, stride=s)
    assert s == 2 and X.shape == (3, len(range(0, T, s)), 2) == (3, 750, 2)
    assert torch.equal(X[0, :, 0], torch.arange(0, 3000, 4, dtype=torch.float32))       # samples 0, 2, 4, ... 1498
    assert torch.equal(mask[1], torch.arange(0, T, 2) < 1203) and torch.equal(mask[2], torch.arange(0, T, 2) < 640)
    assert float(X[2, 320:].abs().max()) == 0.0 and y.dtype == torch.float32


def test_monash_loader_subsamples_long_series(tmp_path):
    import run
    from data_provider.data_factory import data_provider
    from data_provider.ts_reader import write_ts
    d = tmp_path / "Long"
    d.mkdir()
    rng = np.random.RandomState(0)
    for split in ("TRAIN", "TEST"):
        write_ts(str(d / f"Long_{split}.ts"), [rng.randn(1, L) for L in (1500, 1100, 1500)], [1.0, 2.0, 3.0], regression=True)
    a = run.get_args(["--task_name", "regression", "--data", "Monash", "--data_root", str(tmp_path), "--dataset", "Long",
                      "--batch_size", "2"])
    ds, loader = data_provider(a, "train")
    assert (ds.max_seq_len, ds.stride, ds.seq_len) == (1500, 2, 750)
    shapes = [tuple(X.shape) for X, _, _ in loader]
    assert shapes == [(2, 750, 1), (1, 750, 1)]


# ----------------------------------------------------------------------------------------------- C ABI
def test_crps_symbols_declared_bound_exported():
    import ctypes
    from ign_hip import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    for name in ("ign_crps_fwd_bwd", "ign_loss_crps_fwd_bwd_reg"):
        assert re.search(rf"\b{name}\s*\(", hdr) and name in _lib.SIGNATURES
    assert callable(ops.crps_loss) and callable(ops.ign_crps_loss)
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    h = ctypes.CDLL(_lib.lib_path())
    assert hasattr(h, "ign_crps_fwd_bwd") and hasattr(h, "ign_loss_crps_fwd_bwd_reg")
    L = _lib.lib()
    assert L.ign_abi_version() == 1
    # bad arguments: IGN_E_ARG with a message, nothing launched (no device touched)
    assert L.ign_crps_fwd_bwd(None, None, None, None, None, 4, 10, None) == -1001
    assert b"null pointer" in L.ign_last_error()
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.ign_crps_fwd_bwd(p, p, p, p, p, 4, 1, None) == -1001 and b"N=1" in L.ign_last_error()
    assert L.ign_crps_fwd_bwd(p, p, p, p, p, 4, 257, None) == -1001
    assert L.ign_crps_fwd_bwd(p, p, p, p, p, 0, 10, None) == -1001
    assert L.ign_loss_crps_fwd_bwd_reg(p, p, p, p, None, p, p, p, p, p, 4, 300, 1.0, None) == -1001
    assert L.ign_loss_crps_fwd_bwd_reg(p, None, p, p, None, p, p, p, p, p, 4, 10, 1.0, None) == -1001


# ----------------------------------------------------------------------------------------------- torch CRPSLoss
@pytest.mark.parametrize("N", [2, 10, 39])
def test_torch_crps_loss_matches_reference(N):
    from exp.experiment_regression import CRPSLoss
    g = golden("crps_loss")
    z = torch.from_numpy(g[f"n{N}_logits"]).requires_grad_(True)
    loss = CRPSLoss(torch.from_numpy(g[f"n{N}_edges"]))(z, torch.from_numpy(g[f"n{N}_target"]))
    loss.backward()
    assert abs(loss.item() - float(g[f"n{N}_loss"])) <= 1e-6
    np.testing.assert_allclose(z.grad.numpy(), g[f"n{N}_grad"], rtol=1e-5, atol=1e-7)


# ----------------------------------------------------------------------------------------------- CLI + harness
def test_cli_resolves_regression():
    import run
    from exp.experiment_regression import Experiment
    a = run.get_args(["--task_name", "regression", "--data", "Monash"])
    assert run.exp_dict[a.task_name] is Experiment and a.root_path == "./data/UEA_multivariate/BasicMotions"
    assert set(Experiment.model_dict) == {'InterpGN', 'SBM', 'LTS', 'DNN'}


def _write_monash(tmp, n=14, C=3, T=60):
    from data_provider.ts_reader import write_ts
    d = os.path.join(tmp, "Burst")
    os.makedirs(d, exist_ok=True)
    for split, seed in (("TRAIN", 1), ("TEST", 2)):
        rng = np.random.RandomState(seed)
        amp = rng.rand(n) * 4
        X = []
        for i in range(n):
            x = rng.randn(C, T) * 0.3
            x[:, 20:30] += amp[i]
            X.append(x)
        write_ts(os.path.join(d, f"Burst_{split}.ts"), X, amp, regression=True)
    return d


def test_regression_harness_with_oracle_models(tmp_path, monkeypatch):
    import run
    from exp.experiment_regression import Experiment
    from oracle import ign_oracle as O
    _write_monash(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setitem(Experiment.model_dict, 'InterpGN', lambda configs, num_shapelet, shapelet_len:
                        O.OracleIGN(configs, num_shapelet, shapelet_len))
    monkeypatch.setitem(Experiment.model_dict, 'SBM', lambda configs, num_shapelet, shapelet_len:
                        O.OracleSBM(configs, num_shapelet, shapelet_len))
    import utils.tools as T
    real_call = T.EarlyStopping.__call__
    for model in ("InterpGN", "SBM"):
        a = run.get_args(["--task_name", "regression", "--data", "Monash", "--model", model, "--dnn_type", "FCN",
                          "--data_root", str(tmp_path), "--dataset", "Burst", "--train_epochs", "3", "--batch_size", "5",
                          "--seed", "0", "--amp", "--log_interval", "1", "--num_shapelet", "2", "--patience", "1"])
        torch.manual_seed(0)
        e = Experiment(a)
        assert (a.seq_len, a.enc_in, a.num_class) == (60, 3, 10)
        assert e.checkpoint_dir == (f"./checkpoints/{model}/Burst/dnn-FCN_seed-0_k-2_div-0.1_reg-0.1_eps-1.0_"
                                    f"beta-constant_dfunc-euclidean_cls-linear")
        nfeat = 6 * 2 * 3                                        # the 6 x --num_shapelet bank, InterpGN included
        assert e.model.state_dict()[("sbm." if model == "InterpGN" else "") + "output_layer.weight"].shape == (10, nfeat)
        seen = []
        orig = e.validation
        monkeypatch.setattr(e, "validation", lambda: seen.append(orig()) or seen[-1])
        stops = []
        monkeypatch.setattr(T.EarlyStopping, "__call__", lambda self, v, m, p: (stops.append(v), real_call(self, v, m, p))[1])
        e.train()
        assert stops == seen and all(np.isfinite(seen))        # early stopping on the val CRPS itself
        assert os.path.exists(os.path.join(e.checkpoint_dir, "checkpoint.pth"))
        loss, res, df = e.test(result_dir=str(tmp_path / "result"))
        assert isinstance(loss, float) and np.isfinite(loss) and res is None and isinstance(df, dict)
        assert df["pred"].shape == (14, 10) and df["target"].shape == (14,) and df["predicate"].shape == (14, nfeat)
        assert (df["eta"] is not None) == (model == "InterpGN")
        files = glob.glob(str(tmp_path / "result" / f"Burst-0-{model}-*.csv"))
        assert len(files) >= 1
        cols = set(open(sorted(files)[-1]).readline().strip().split(","))
        assert {"model", "dataset", "seed", "test_loss", "epoch_stop", "eta_mean", "eta_std", "w_sum_10", "w_mean_10", "w_sum_5",
                "w_mean_5", "w_sum_1", "w_mean_1", "w_max", "w_gini_clip", "w_gini_abs"} <= cols
