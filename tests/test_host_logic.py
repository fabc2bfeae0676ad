"""CPU tests of the host side: CLI contract, .ts reader, UEA loader / collate, synthetic + npy providers,
EarlyStopping, the Experiment harness (with the CPU oracle standing in for the GPU models), and the C ABI."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, make_cfg

import speech_imagery_eeg_amd  # noqa: F401  (puts the package directory on sys.path)


# ----------------------------------------------------------------------------------------------- CLI
def test_cli_flags_match_reference():
    """Every flag of the reference's run.py exists with the same default / action (tests/golden/run_flags.json)."""
    import run
    ref = json.load(open(os.path.join(GOLDEN, "run_flags.json")))
    parser = run.build_parser()
    mine = {a.option_strings[0]: a for a in parser._actions if a.option_strings and a.option_strings[0] != '-h'}
    repaired = {"--data": "UEA", "--data_root": "./data/UEA_multivariate", "--json_path": "./json/textmaps.json"}
    for flag, spec in ref.items():
        assert flag in mine, f"missing flag {flag}"
        act = mine[flag]
        if flag in repaired:
            assert act.default == repaired[flag]          # documented repair of SURVEY D2
            continue
        implied = {"store_true": False, "store_false": True}.get(spec.get("action"))
        assert act.default == spec.get("default", implied), flag
        if spec.get("action") == "store_false":
            assert act.const is False and act.default is True
        if spec.get("action") == "store_true":
            assert act.const is True
    a = run.get_args(["--amp"])
    assert a.amp is False                                   # the inverted flag
    assert run.get_args([]).amp is True
    assert set(run.exp_dict) == {"classification", "regression"}


def test_registries():
    from exp.experiment_classification import Experiment, compute_beta
    from models.InterpGN import dnn_dict
    from data_provider.data_factory import data_dict
    assert set(Experiment.model_dict) == {'InterpGN', 'SBM', 'LTS', 'DNN', 'EEGCNN'}
    assert set(dnn_dict) == {'FCN', 'Transformer', 'TimesNet', 'PatchTST', 'ResNet'}
    assert {'UEA', 'EEG', 'EEG3'} <= set(data_dict)
    assert compute_beta(0, 10, 'cosine') == 1.0 and abs(compute_beta(5, 10, 'cosine') - 0.5) < 1e-12
    assert compute_beta(5, 10, 'linear') == 0.5 and compute_beta(3, 10, 'constant') == 1
    import model, data_factory            # the reference's directory names resolve to the same packages (D1)
    import models, data_provider
    assert model is models and data_factory is data_provider


def test_state_dict_keys_ign():
    from models.InterpGN import InterpGN
    m = InterpGN(make_cfg(enc_in=122, seq_len=1000, num_class=3))
    sd = m.state_dict()
    assert [tuple(sd[f"sbm.shapelets.{i}.weights"].shape) for i in range(4)] == \
        [(5, 122, 100), (5, 122, 200), (5, 122, 300), (5, 122, 500)]
    assert tuple(sd["sbm.output_layer.weight"].shape) == (3, 2440)
    assert tuple(sd["deep_model.block1.0.weight"].shape) == (128, 122, 8)
    assert "deep_model.block3.1.num_batches_tracked" in sd and tuple(sd["deep_model.fc.weight"].shape) == (3, 128)
    assert sum(p.numel() for p in m.parameters()) == 1_067_315          # SURVEY K12 (probe of the reference)


# ----------------------------------------------------------------------------------------------- data
def _write_bm(tmp, n=12, C=6, T=100, ragged=False):
    from data_provider.ts_reader import write_ts
    rng = np.random.RandomState(0)
    d = os.path.join(tmp, "BasicMotions")
    os.makedirs(d, exist_ok=True)
    classes = ["badminton", "running", "standing", "walking"]
    for split, seed in (("TRAIN", 1), ("TEST", 2)):
        rng = np.random.RandomState(seed)
        X = [rng.randn(C, T - (i % 3) * 10 if ragged else T) for i in range(n)]
        y = [classes[i % 4] for i in range(n)]
        write_ts(os.path.join(d, f"BasicMotions_{split}.ts"), X, y, "BasicMotions", classes)
    return d


def test_ts_reader_roundtrip_and_missing(tmp_path):
    from data_provider.ts_reader import load_ts, write_ts, TsFormatError
    X = [np.arange(12, dtype=float).reshape(2, 6), np.ones((2, 6))]
    p = str(tmp_path / "a.ts")
    write_ts(p, X, ["u", "v"])
    cases, labels, meta = load_ts(p)
    assert labels == ["u", "v"] and meta["dimensions"] == "2"
    np.testing.assert_array_equal(np.stack(cases[0]), X[0])
    with open(p, "a") as f:
        f.write("1,?,3:4,5,6:u\n")
    cases, labels, _ = load_ts(p)
    assert np.isnan(cases[2][0][1]) and labels[2] == "u"
    bad = str(tmp_path / "bad.ts")
    open(bad, "w").write("@problemName x\n1,2,3:a\n")
    with pytest.raises(TsFormatError):
        load_ts(bad)


def test_uea_loader_and_collate(tmp_path):
    from data_provider.data_loader import UEAloader
    from data_provider.uea import collate_fn, padding_mask
    d = _write_bm(str(tmp_path), ragged=True)
    tr = UEAloader(d, flag="train")
    va = UEAloader(d, flag="val")          # no VAL file: upstream uses TEST
    te = UEAloader(d, flag="TEST")
    assert len(tr) == len(va) == len(te) == 12
    assert (tr.enc_in, tr.max_seq_len, tr.num_classes) == (6, 100, 4)
    x0, y0 = tr[0]
    assert x0.shape == (100, 6) and y0.dtype == torch.int8 and y0.shape == (1,)
    assert tr[1][0].shape == (90, 6)
    allv = tr.feature_df
    np.testing.assert_allclose(allv.mean(0), 0, atol=1e-9)           # standardised over all rows
    X, y, m = collate_fn([tr[0], tr[1], tr[2]], max_len=95)
    assert X.shape == (3, 95, 6) and X.dtype == torch.float32 and y.shape == (3, 1) and m.shape == (3, 95)
    assert m[0].all() and m[1, :90].all() and not m[1, 90:].any()      # clip (100 -> 95) and pad (90 -> 95)
    assert float(X[1, 90:].abs().sum()) == 0.0
    assert padding_mask(torch.tensor([2, 0, 3])).tolist() == [[True, True, False], [False] * 3, [True] * 3]


def test_normalizer_variants():
    from data_provider.uea import Normalizer, interpolate_missing, subsample
    v = np.array([[1., 10.], [3., 30.], [5., 20.], [7., 40.]])
    ids = np.array([0, 0, 1, 1])
    s = Normalizer('standardization').normalize(v)
    np.testing.assert_allclose(s.std(0, ddof=1), 1, rtol=1e-12)
    mm = Normalizer('minmax').normalize(v)
    assert mm.min() == 0 and abs(mm.max() - 1) < 1e-12
    ps = Normalizer('per_sample_std').normalize(v, ids)
    np.testing.assert_allclose(ps[:2].mean(0), 0, atol=1e-12)
    with pytest.raises(NameError):
        Normalizer('nope').normalize(v)
    np.testing.assert_allclose(interpolate_missing([np.nan, 1, np.nan, 3, np.nan]), [1, 1, 2, 3, 3])
    assert len(subsample(np.arange(300))) == 150 and len(subsample(np.arange(10))) == 10


def test_synthetic_and_npy_providers(tmp_path):
    from data_provider.synthetic import SyntheticEEG
    from data_provider.eeg_npy import EEGNpyDataset3Class, per_sample_standardise, split_indices
    a, b = SyntheticEEG(flag='train', n=16, seq_len=50, enc_in=5), SyntheticEEG(flag='train', n=16, seq_len=50, enc_in=5)
    assert torch.equal(a.x, b.x) and torch.equal(a.y, b.y)              # deterministic across processes / ranks
    assert a[0][0].shape == (50, 5) and a[0][1].dtype == torch.int8
    rng = np.random.RandomState(0)
    X = (rng.randn(40, 4, 30) * 20 + 100).astype(np.float32)
    np.save(tmp_path / "X.npy", X)
    np.save(tmp_path / "y.npy", rng.randint(0, 39, 40))
    parts = [EEGNpyDataset3Class(str(tmp_path), f) for f in ("train", "val", "test")]
    assert [len(p) for p in parts] == [28, 4, 8] and parts[0].num_classes == 3       # 70 / 10 / 20
    idx = np.concatenate([split_indices(40, f) for f in ("train", "val", "test")])
    assert sorted(idx.tolist()) == list(range(40))
    x, y = parts[0][0]
    assert x.shape == (30, 4) and 0 <= int(y) < 3
    z = per_sample_standardise(X[:2])
    np.testing.assert_allclose(z.mean(-1), 0, atol=1e-5)
    with pytest.raises(FileNotFoundError):
        EEGNpyDataset3Class(str(tmp_path / "nope"), "train")


def test_tensor_batch_loader_yields_the_collate_contract():
    """data_provider's in-memory fast path (TensorBatchLoader, `--data SYNTH`) against DataLoader + collate_fn on the same data set
    and order: same tensors, dtypes and shapes, ragged last batch included; a sampler and a shuffled epoch cover every index once."""
    from torch.utils.data import DataLoader
    from data_provider.device_prefetch import TensorBatchLoader
    from data_provider.synthetic import SyntheticEEG
    from data_provider.uea import collate_fn
    ds = SyntheticEEG(flag='val', n=21, seq_len=30, enc_in=4)
    ref = list(DataLoader(ds, batch_size=8, shuffle=False, collate_fn=lambda b: collate_fn(b, max_len=30)))
    got = list(TensorBatchLoader(ds, 8, shuffle=False))
    assert len(got) == len(ref) == len(TensorBatchLoader(ds, 8)) == 3
    for (x, y, m), (xr, yr, mr) in zip(got, ref):
        assert x.dtype == xr.dtype and y.dtype == yr.dtype and m.dtype == mr.dtype
        assert torch.equal(x, xr) and torch.equal(y, yr) and torch.equal(m, mr)
    torch.manual_seed(0)
    seen = torch.cat([y for _, y, _ in TensorBatchLoader(ds, 8, shuffle=True)])
    assert seen.shape == (21, 1)
    idx = [20, 3, 3, 7]
    xs = torch.cat([x for x, _, _ in TensorBatchLoader(ds, 3, sampler=idx)])
    assert torch.equal(xs, ds.x[idx])


# ----------------------------------------------------------------------------------------------- harness
def test_early_stopping_contract(tmp_path):
    from utils.tools import EarlyStopping, convert_to_hms, gini_coefficient
    m = torch.nn.Linear(2, 2)
    es = EarlyStopping(patience=2)
    for v in (-0.5, -0.6, -0.6, -0.55, -0.58):   # harness passes -val_acc; an equal score counts as improvement
        es(v, m, str(tmp_path))
    assert es.early_stop and es.counter == 2 and os.path.exists(tmp_path / "checkpoint.pth")
    assert set(torch.load(tmp_path / "checkpoint.pth", weights_only=True)) == {"weight", "bias"}
    assert convert_to_hms(3725) == "01:02:05"
    assert abs(gini_coefficient(np.array([[1., 1., 1., 1.]]))) < 1e-12


def _harness_args(tmp, model, **kw):
    import run
    a = run.get_args(["--model", model, "--dnn_type", "FCN", "--data", "UEA", "--data_root", tmp, "--dataset",
                      "BasicMotions", "--train_epochs", "2", "--batch_size", "6", "--seed", "0", "--amp",
                      "--log_interval", "1", "--num_shapelet", "2"])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_experiment_harness_with_oracle_models(tmp_path, monkeypatch):
    """Host logic of Experiment (loaders -> params -> loss composition -> Adam -> early stopping -> checkpoint ->
    test) exercised on CPU with the oracle models in the registry (the GPU models need the HIP library + a GPU)."""
    from exp.experiment_classification import Experiment
    from oracle import ign_oracle as O
    d = _write_bm(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)      # on CPU even where a GPU is visible
    monkeypatch.setitem(Experiment.model_dict, 'InterpGN', lambda cfg: O.OracleIGN(cfg))
    monkeypatch.setitem(Experiment.model_dict, 'SBM', lambda configs, num_shapelet, shapelet_len:
                        O.OracleSBM(configs, num_shapelet, shapelet_len))
    for model in ("InterpGN", "SBM"):
        a = _harness_args(str(tmp_path), model)
        torch.manual_seed(0)
        e = Experiment(a)
        assert (a.seq_len, a.enc_in, a.num_class) == (100, 6, 4)          # read from the dataset, not EEG defaults
        assert e.checkpoint_dir == (f"./checkpoints/{model}/BasicMotions/dnn-FCN_seed-0_k-2_div-0.1_reg-0.1_eps-1.0_"
                                    f"beta-constant_dfunc-euclidean_cls-linear")
        e.train()
        assert os.path.exists(os.path.join(e.checkpoint_dir, "checkpoint.pth"))
        loss, res, df = e.test(result_dir=str(tmp_path / "result"))
        assert res.preds.shape == (12,) and 0.0 <= res.accuracy <= 1.0 and np.isfinite(loss)
        # the test summary the reference intends (exp:500-532): one CSV row with these columns
        import glob
        files = glob.glob(str(tmp_path / "result" / f"BasicMotions-0-{model}-*.csv"))
        assert len(files) >= 1 and df is not None
        cols = set(open(files[0]).readline().strip().split(","))
        assert {"model", "dataset", "seed", "test_accuracy", "epoch_stop", "shapelet_score", "w_count_0.5", "w_ratio_0.1",
                "w_max", "w_gini_clip", "w_gini_abs", "eta_mean", "eta_std"} <= cols
        assert abs(float(df["test_accuracy"][0]) - res.accuracy) < 1e-12 and 0.0 <= float(df["w_gini_abs"][0]) <= 1.0
        nfeat = 4 * 5 * 6 if model == "InterpGN" else 6 * 2 * 6            # D4: IGN ignores --num_shapelet
        assert res.p.shape == (12, nfeat) and res.w.shape == (4, nfeat) and len(res.shapelets) == nfeat // 6 * 6
        if model == "InterpGN":
            assert res.eta.shape == (12, 1) and res.dnn_preds.shape == (12, 4)


def test_product_models_refuse_cpu(tmp_path, monkeypatch):
    """No silent CPU fallback: the real registry raises on a CPU tensor."""
    from exp.experiment_classification import Experiment
    from ign_hip._lib import IgnError
    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    _write_bm(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    e = Experiment(_harness_args(str(tmp_path), "InterpGN"))
    with pytest.raises(IgnError):
        e.train()


# ----------------------------------------------------------------------------------------------- C ABI
def test_abi_exports_every_declared_symbol():
    from ign_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "ign_abi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ign_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SIGNATURES), f"header vs binding: {declared ^ set(_lib.SIGNATURES)}"
    path = _lib.lib_path()
    if not os.path.exists(path):
        pytest.skip("libign_hip.so not built (run __graft_entry__.build())")
    h = ctypes.CDLL(path)                      # loads without a GPU; no compute call is made
    for name in declared:
        assert hasattr(h, name), f"{name} not exported"
    assert _lib.lib().ign_abi_version() == 1
    # argument errors are reported without touching a device
    assert _lib.lib().ign_instnorm_fwd(None, None, None, 1, 1, 1, 1e-8, None) == -1001
    assert b"null pointer" in _lib.lib().ign_last_error()


def test_raw_chisco_items_and_prefetcher_passthrough(tmp_path):
    """The device input pipeline's host side: raw (C,T) items + collate_raw carry exactly the data whose standardised,
    transposed form the CPU path yields; on a CPU device the prefetcher is a pass-through that applies the transform."""
    import numpy as np
    import torch
    import speech_imagery_eeg_amd  # noqa: F401
    from data_provider.device_prefetch import DevicePrefetcher
    from data_provider.eeg_npy import EEGNpyDataset3Class, collate_raw, per_sample_standardise
    from data_provider.uea import collate_fn
    rng = np.random.RandomState(0)
    X = (rng.randn(30, 5, 40) * 50 + 1e4).astype(np.float32)
    y = rng.randint(0, 39, size=30)
    np.save(tmp_path / "X.npy", X)
    np.save(tmp_path / "y.npy", y)
    cpu = EEGNpyDataset3Class(str(tmp_path), flag="train")
    raw = EEGNpyDataset3Class(str(tmp_path), flag="train", raw=True)
    assert len(cpu) == len(raw) == 21 and raw.num_classes == 3
    xb, yb, none = collate_raw([raw[i] for i in range(4)])
    xc, yc, mask = collate_fn([cpu[i] for i in range(4)], max_len=40)
    assert none is None and xb.shape == (4, 5, 40) and torch.equal(yb, yc) and bool(mask.all())
    ref = torch.from_numpy(per_sample_standardise(xb.numpy())).permute(0, 2, 1)
    assert torch.allclose(ref, xc, atol=1e-6)

    def to_btc(batch):        # the CPU twin of standardise_raw_batch
        x, yy, _ = batch
        xs = torch.from_numpy(per_sample_standardise(x.numpy())).permute(0, 2, 1).contiguous()
        return xs, yy, torch.ones(xs.shape[0], xs.shape[1], dtype=torch.bool)

    loader = torch.utils.data.DataLoader(raw, batch_size=8, shuffle=False, collate_fn=collate_raw)
    pf = DevicePrefetcher(loader, "cpu", transform=to_btc)
    assert len(pf) == 3 and pf.dataset is raw
    got = list(pf)
    want = list(torch.utils.data.DataLoader(cpu, batch_size=8, shuffle=False, collate_fn=lambda b: collate_fn(b, max_len=40)))
    assert len(got) == len(want) == 3
    for (a, b_, m), (c, d, n) in zip(got, want):
        assert torch.allclose(a, c, atol=1e-6) and torch.equal(b_, d) and torch.equal(m, n)


def test_abi_argument_errors_of_the_gemm_and_attention_entry_points():
    """Argument checking happens before any launch: callable without a GPU, returns the documented codes and a reason."""
    import ctypes
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built (run __graft_entry__.build())")
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ARG, UNSUP = -1001, -1002
    # weight gradient, split-bf16: tap counts without an instantiated kernel / k = 1 with odd channel counts
    assert L.ign_clconv_wgrad_x6(p, 0, p, None, None, p, p, 2, 50, 8, 8, 4, None) == UNSUP
    assert b"k in" in L.ign_last_error()
    assert L.ign_clconv_wgrad_x6(p, 0, p, None, None, p, p, 1, 50, 6, 8, 1, None) == UNSUP
    assert L.ign_clconv_wgrad_bf16(None, 0, p, None, None, p, p, 2, 50, 8, 8, 3, None) == ARG
    assert L.ign_clconv_wgrad_x6_workspace_bytes(2, 50, 8, 8, 4) == 0
    assert L.ign_clconv_wgrad_x6_workspace_bytes(1, 4096, 64, 64, 1) > 0
    # forward GEMMs: more than 16 taps / a prologue with only one of its two vectors
    assert L.ign_clconv_fwd_x6(p, p, None, None, None, p, None, 1, 64, 8, 8, 17, None) == UNSUP
    assert L.ign_clconv_fwd_bf16(p, p, None, p, None, p, None, 1, 64, 8, 8, 3, None) == ARG
    # attention: head sizes, alignment, strides
    for fn in (L.ign_attn_fwd_x6, L.ign_attn_fwd_bf16):
        assert fn(p, p, p, p, p, 1, 8, 8, 1, 48, 384, 48, 384, 48, 384, 48, 0.1, None) == UNSUP
        assert fn(p, p, p, p, None, 1, 8, 8, 1, 64, 512, 64, 512, 64, 512, 64, 0.1, None) == ARG
        assert fn(p, p, p, p, p, 1, 8, 8, 1, 64, 512, 62, 512, 64, 512, 64, 0.1, None) == ARG
    assert b"stride" in L.ign_last_error()
    for fn in (L.ign_attn_bwd_x6, L.ign_attn_bwd_bf16):
        assert fn(p, p, p, p, p, p, p, p, p, p, 1, 8, 8, 1, 24, 192, 24, 192, 24, 192, 24, 0.1, None) == UNSUP
        assert fn(p, p, p, p, p, p, p, p, None, p, 1, 8, 8, 1, 64, 512, 64, 512, 64, 512, 64, 0.1, None) == ARG


@pytest.mark.parametrize("name", ["ign_adam_step", "ign_adam_step_clip", "ign_adam_step_dev", "ign_adam_step_clip_dev"])
def test_adam_entry_points_refuse_a_parameter_pointer_that_is_not_16_byte_aligned(name):
    """All four read and write 16 bytes at a time; the check precedes any launch, so the address is never dereferenced."""
    import ctypes
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built (run __graft_entry__.build())")
    L = _lib.lib()
    buf = (ctypes.c_float * 72)(*range(72))
    base = (ctypes.addressof(buf) + 15) & ~15
    at = lambda floats: ctypes.c_void_p(base + 4 * floats)
    args = [at(1), at(16), at(32), at(48), 8, 5e-3, 0.9, 0.999, 1e-8]
    args += [at(64), at(64)] if name.endswith("_dev") else [1]
    if "_clip" in name:
        args.append(at(64))
    assert getattr(L, name)(*args, None) == -1001
    err = L.ign_last_error()
    assert err.startswith(name.encode() + b":") and b"16-byte aligned" in err
    assert list(buf) == [float(i) for i in range(72)]
    args[0] = None
    assert getattr(L, name)(*args, None) == -1001 and L.ign_last_error().startswith(name.encode() + b": null pointer")


@pytest.mark.parametrize("name", ["FCN", "ResNet", "PatchTST", "TimesNet", "Transformer", "EEGCNN"])
def test_every_deep_expert_refuses_cpu_tensors(name):
    """No silent CPU path anywhere in the product models: a CPU tensor raises IgnError in every deep expert / baseline."""
    import contextlib, io
    from conftest import make_cfg
    from ign_hip._lib import IgnError
    from models.InterpGN import dnn_dict
    cfg = make_cfg(seq_len=96, d_model=16, d_ff=16, top_k=2, num_kernels=2, n_heads=1)
    x = torch.randn(2, 96, 6)
    mask = torch.ones(2, 96)
    with contextlib.redirect_stdout(io.StringIO()):
        if name == "EEGCNN":
            from models.eegcnn import EEGCNNTransformer
            m, args = EEGCNNTransformer(make_cfg(enc_in=6, seq_len=1000, num_class=3, c_out=3, d_model=64)), (torch.randn(2, 6, 1000),)
        else:
            m, args = dnn_dict[name](cfg), (x, mask, None, None)
        with pytest.raises(IgnError):
            m(*args)
