"""Host side of the spatial filter stage (--eeg_spatial; utils/eeg_spatial.py): the flag's parser, the composition of reference and
montage, the numpy restatement of the apply and Gram rules, the Euclidean alignment fitted through the numpy path, the data set /
loader wiring on temporary shards, and the three ABI symbols with their refusals (which return before anything is launched, so they
need no device).  The case tables are tests/eeg_spatial_cases.py; the device side is tests/test_gpu_eeg_spatial.py."""
import ctypes
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from eeg_spatial_cases import APPLY_CASES, S, apply_case, check_apply, gram_case, identity_expectation, write_shards


# ------------------------------------------------------------------------------------------------------------------ parser
def test_parser_accepts_every_key_in_any_order(tmp_path):
    s = S()
    m = tmp_path / "m.npy"
    np.save(m, np.eye(4))
    assert s.parse_eeg_spatial("ref=car") == s.EEGSpatialSpec(ref='car')
    assert s.parse_eeg_spatial("align=euclid") == s.EEGSpatialSpec(align='euclid')
    full = s.parse_eeg_spatial(f"rtol=1e-4, align=euclid ,matrix={m},ref=car")
    assert full == s.EEGSpatialSpec(ref='car', matrix=str(m), align='euclid', rtol=1e-4) and full.active
    assert s.parse_eeg_spatial(full) is full
    assert s.parse_eeg_spatial(full.text) == full                          # the text written to eeg_spatial.npz parses back
    assert s.EEGSpatialSpec().rtol == 1e-6
    for off in ("none", "", None, "NONE", "  "):
        spec = s.parse_eeg_spatial(off)
        assert spec == s.EEGSpatialSpec() and not spec.active and spec.text == 'none'


@pytest.mark.parametrize("text,msg", [
    ("car", "is not one of"), ("ref", "is not one of"), ("reference=car", "is not one of"), ("ref=car,fit", "is not one of"),
    ("ref=car,ref=car", "ref given twice"), ("align=euclid,rtol=1e-3,align=euclid", "align given twice"),
    ("ref=laplace", "is not car"), ("align=riemann", "is not euclid"), ("align=", "is not euclid"),
    ("rtol=0", "outside"), ("rtol=1", "outside"), ("rtol=-1e-3", "outside"), ("rtol=nan", "outside"), ("rtol=small", "not a number"),
    ("matrix=/no/such/file.npy", "no such file"), ("matrix=", "no such file"),
])
def test_parser_refusals(text, msg):
    with pytest.raises(ValueError, match=msg):
        S().parse_eeg_spatial(text)


def test_run_flag_and_its_refusal(tmp_path):
    import speech_imagery_eeg_amd  # noqa: F401
    import run as driver
    args = driver.get_args(["--data", "EEG3", "--data_root", str(tmp_path), "--eeg_spatial", "ref=car,align=euclid"])
    assert args.eeg_spatial == "ref=car,align=euclid"
    assert driver.get_args(["--data", "EEG3", "--data_root", str(tmp_path)]).eeg_spatial == 'none'
    with pytest.raises(ValueError, match="--eeg_spatial"):
        driver.get_args(["--data", "SYNTH", "--eeg_spatial", "ref=car"])
    with pytest.raises(ValueError, match="given twice"):
        driver.get_args(["--data", "EEG", "--data_root", str(tmp_path), "--eeg_spatial", "ref=car,ref=car"])
    assert "--eeg_spatial" in driver.build_parser().format_help()
    from exp.experiment_classification import Experiment
    assert 'eeg_spatial' in Experiment.SUMMARY_ARGS


# ----------------------------------------------------------------------------------------------------------------- compose
def test_compose_car_is_a_projector_and_matrix_shapes_are_checked(tmp_path):
    s = S()
    for Cin in (5, 122):
        H = s.compose("ref=car", Cin)
        assert H.shape == (1, Cin, Cin) and H.dtype == np.float64
        assert float(np.abs(H[0].sum(axis=1)).max()) <= 1e-15
        Hl = H[0].astype(np.longdouble)              # the product in extended precision: a float64 dot of 122 terms rounds at 1e-15 itself
        assert float(np.abs(Hl @ Hl - Hl).max()) <= 1e-15
    assert np.array_equal(s.compose("align=euclid", 4)[0], np.eye(4))
    rng = np.random.RandomState(0)
    M2, M3 = rng.randn(3, 5), rng.randn(2, 3, 5)
    assert np.array_equal(s.compose("none", 5, M2), M2[None])
    W = s.compose("ref=car", 5, M3)
    assert W.shape == (2, 3, 5) and np.allclose(W, M3 @ (np.eye(5) - 0.2), rtol=0, atol=1e-15)
    assert float(np.abs(W.sum(axis=-1)).max()) < 1e-14                      # behind CAR every virtual channel ignores a common offset
    p = tmp_path / "m.npy"
    np.save(p, M2)
    assert np.array_equal(s.compose(f"matrix={p}", 5), M2[None])            # read from the spec's file
    for bad in (rng.randn(3, 4), rng.randn(5), rng.randn(2, 2, 3, 5), np.zeros((0, 5))):
        with pytest.raises(ValueError, match="matrix of shape"):
            s.compose("ref=car", 5, bad)
    with pytest.raises(ValueError, match="not finite"):
        s.compose("none", 2, np.array([[1.0, np.nan]]))
    with pytest.raises(ValueError, match="beyond"):
        s.compose("none", 2, np.zeros((s.MAX_GROUPS + 1, 1, 2)))
    with pytest.raises(ValueError, match="input channels"):
        s.compose("ref=car", s.MAX_CHANNELS + 1)
    assert s.needs_groups("align=euclid") and s.needs_groups("ref=car", M3) and not s.needs_groups("ref=car", M2)


# ------------------------------------------------------------------------------------------------------- the rule in numpy
@pytest.mark.parametrize("label", list(APPLY_CASES))
def test_spatial_numpy_is_the_product_and_its_fp32_form_meets_both_bounds(label):
    s = S()
    k = apply_case(label)
    y64 = s.spatial_numpy(k["x"], k["W"], k["gid"])
    assert y64.dtype == np.float64
    assert float(np.abs(y64 - k["y64"]).max()) <= 1e-12 * float(np.abs(k["y64"]).max())
    y32 = s.spatial_numpy(k["x"], k["W"], k["gid"], dtype=np.float32)
    assert y32.dtype == np.float32
    check_apply(label, y32)
    if k["W"].shape[0] == 1:                                                # a 2-D W is one group; one item is a batch of one
        assert np.array_equal(s.spatial_numpy(k["x"], k["W"][0], dtype=np.float32), y32)
        assert np.array_equal(s.spatial_numpy(k["x"][0], k["W"][0], dtype=np.float32), y32[0])


@pytest.mark.parametrize("label", list(APPLY_CASES))
def test_identity_returns_x_exactly_in_the_fp32_form(label):
    """W = I: bit for bit x on every element whose pivot subtraction is exact, and bit for bit fl(fl(x - p) + p) everywhere.  Under
    the recipe x - p is inexact on 117 of 84000 elements of E_unused_group (2 rows whose offset is below their signal) and 1102 of
    402844 of F_real_row (3 rows), and on none of the other cases."""
    s = S()
    x = apply_case(label)["x"]
    want, exact = identity_expectation(x)
    y = s.spatial_numpy(x, np.eye(x.shape[1], dtype=np.float32), dtype=np.float32)
    assert np.array_equal(y, want)
    assert np.array_equal(y[exact], x[exact]) and exact.mean() > 0.99
    if label not in ("E_unused_group", "F_real_row"):
        assert exact.all() and np.array_equal(y, x)


def test_spatial_numpy_out_of_range_groups_and_shape_checks():
    s = S()
    k = apply_case("C_tile_crossing")
    y = s.spatial_numpy(k["x"], k["W"], [1, 2, -1], dtype=np.float32)
    ok = s.spatial_numpy(k["x"], k["W"], k["gid"], dtype=np.float32)
    assert np.array_equal(y[0], ok[0]) and not y[1].any() and not y[2].any()
    with pytest.raises(ValueError):
        s.spatial_numpy(k["x"], np.zeros((7, 32)))


def test_gram_numpy_restates_the_rule():
    s = S()
    k = gram_case("B_empty_group")
    x = k["x"].astype(np.float64)
    z = x - x.mean(axis=-1, keepdims=True)                                  # in exact arithmetic the pivot cancels
    want = np.zeros_like(k["gram64"])
    for b, g in enumerate(k["gid"]):
        want[g] += z[b] @ z[b].T
    assert np.allclose(k["gram64"], want, rtol=1e-9, atol=0) and k["count"].tolist() == [2, 0, 2]
    assert not k["gram64"][1].any() and np.array_equal(k["gram64"], k["gram64"].transpose(0, 2, 1))
    g1, c1 = s.gram_numpy(k["x"], None, 1)
    assert np.allclose(g1[0], want.sum(axis=0), rtol=1e-9, atol=0) and c1.tolist() == [4]


# ---------------------------------------------------------------------------------------------------------------- the fit
def _trials(groups=3, per_group=(5, 4, 6), C=6, T=200, seed=3):
    """raw trials of `groups` subjects, each a fixed mixing (condition number 30) of white sources, on large offsets, in batches of 4"""
    rng = np.random.RandomState(seed)
    mix = []
    for g in range(groups):
        q1, _ = np.linalg.qr(rng.randn(C, C))
        q2, _ = np.linalg.qr(rng.randn(C, C))
        mix.append(q1 @ np.diag(np.geomspace(1.0, 30.0, C)) @ q2.T)
    gid = np.concatenate([np.full(n, g) for g, n in enumerate(per_group)]).astype(np.int32)
    rng.shuffle(gid)
    X = np.stack([mix[g] @ rng.randn(C, T) * 10.0 + rng.uniform(-2e4, 2e4, size=(C, 1)) for g in gid]).astype(np.float32)
    batches = [(torch.from_numpy(X[i:i + 4]), None, torch.from_numpy(gid[i:i + 4])) for i in range(0, len(gid), 4)]
    return X, gid, batches


def _covariances(X, gid, W0, groups):
    """R_g of the rule in float64, computed here from the raw trials: mean over the group's trials of W0 z z^T W0^T / T"""
    X = X.astype(np.float64)
    z = X - X.mean(axis=-1, keepdims=True)
    R = np.zeros((groups, W0.shape[1], W0.shape[1]))
    for g in range(groups):
        sel = z[gid == g]
        for t in sel:
            v = W0[g if W0.shape[0] > 1 else 0] @ t
            R[g] += v @ v.T
        R[g] /= max(len(sel), 1) * X.shape[-1]
    return R


@pytest.mark.parametrize("spec", ["align=euclid", "ref=car,align=euclid"])
def test_fit_alignment_whitens_every_group(spec):
    """A W0 R_g W0^T A = I (the projector onto the kept subspace behind CAR) to 1e-9 for the float64 W = A W0 -- a float64 identity
    at this condition number (30^2 per covariance); the fp32 W that is returned is that matrix rounded once."""
    s = S()
    X, gid, batches = _trials()
    W0 = s.compose(spec, 6)
    W, info = s.fit_alignment(batches, W0, 3, 1e-6, return_info=True)
    assert W.shape == (3, 6, 6) and W.dtype == np.float32 and info["count"].tolist() == [5, 4, 6] and info["empty"] == []
    assert np.array_equal(W, info["W64"].astype(np.float32))
    R = _covariances(X, gid, W0, 3)
    H = W0[0]
    for g in range(3):
        A = info["W64"][g] @ np.linalg.pinv(W0[0])
        got = A @ R[g] @ A.T
        assert float(np.abs(got - (H if "car" in spec else np.eye(6))).max()) <= 1e-9, (g, got)
        assert float(np.abs(info["R"][g] - R[g]).max()) <= 1e-9 * float(np.abs(R[g]).max())
    # the aligned trials of every group have the identity as their mean covariance: what Euclidean alignment is for
    if "car" not in spec:
        Ra = _covariances(X, gid, info["W64"], 3)
        assert float(np.abs(Ra - np.eye(6)).max()) <= 1e-9
    W2 = s.fit_alignment(batches, W0, 3, 1e-6)                              # two fits, equal bits
    assert W2.tobytes() == W.tobytes()
    Wn = s.fit_alignment([(b[0].numpy(), None, b[2].numpy()) for b in batches], W0, 3, 1e-6)        # arrays as well as tensors
    assert Wn.tobytes() == W.tobytes()


def test_fit_alignment_gives_an_empty_group_the_pooled_matrix():
    s = S()
    X, gid, batches = _trials()
    notices = []
    W, info = s.fit_alignment(batches, np.eye(6)[None], 5, 1e-6, notice=notices.append, return_info=True)
    assert info["empty"] == [3, 4] and len(notices) == 1 and "pooled" in notices[0]
    z = X.astype(np.float64) - X.astype(np.float64).mean(axis=-1, keepdims=True)
    pooled = s.inverse_root(np.einsum('bit,bjt->ij', z, z) / (len(X) * X.shape[-1]), 1e-6)
    for g in (3, 4):
        assert float(np.abs(info["W64"][g] - pooled).max()) <= 1e-9 * float(np.abs(pooled).max())
    assert W[3].tobytes() == W[4].tobytes() and W[3].tobytes() != W[0].tobytes()
    one = s.fit_alignment(batches, np.eye(6)[None], 1, 1e-6)               # one group: the pooled matrix itself
    assert float(np.abs(one[0] - pooled).max()) <= 1e-6 * float(np.abs(pooled).max())
    with pytest.raises(ValueError, match="groups"):
        s.fit_alignment(batches, np.zeros((2, 6, 6)), 3)
    with pytest.raises(ValueError, match="no training trial"):
        s.fit_alignment([], np.eye(6)[None], 3)


def test_inverse_root_drops_what_rtol_says_is_not_information():
    s = S()
    q, _ = np.linalg.qr(np.random.RandomState(0).randn(4, 4))
    R = q @ np.diag([4.0, 1.0, 1e-3, 1e-9]) @ q.T
    A = s.inverse_root(R, 1e-6)
    assert np.allclose(A @ R @ A, q[:, :3] @ q[:, :3].T, atol=1e-9)
    assert np.array_equal(A, A.T)
    assert not s.inverse_root(np.zeros((3, 3)), 1e-6).any()


# ----------------------------------------------------------------------------------------------------------- the data path
def _ns(tmp_path, **kw):
    base = dict(task_name="classification", data="EEG", root_path=str(tmp_path), batch_size=8, num_workers=0, seed=0,
                target_channels=4, target_timepoints=40)
    base.update(kw)
    return Namespace(**base)


def test_default_leaves_the_loader_as_it_is(tmp_path):
    import speech_imagery_eeg_amd  # noqa: F401
    from data_provider.data_factory import data_provider, ordered_loader
    from data_provider.eeg_npy import collate_raw
    write_shards(str(tmp_path))
    os.remove(tmp_path / "subject.npy")
    for kw in ({}, dict(eeg_spatial="none"), dict(eeg_spatial=None)):
        ds, loader = data_provider(_ns(tmp_path, device_standardise=True, **kw), "train")
        assert loader.collate_fn is collate_raw and loader.eeg_chain is ds.chain and loader.eeg_chain.stages == []
        assert ds.spatial is None and ds.enc_in == 6
        assert ordered_loader(loader).eeg_chain is ds.chain
        assert len(ds[0]) == 2 and len(next(iter(loader))) == 3 and next(iter(loader))[2] is None
        ds, loader = data_provider(_ns(tmp_path, device_standardise=False, **kw), "train")
        assert loader.eeg_chain is None and ds.spatial is None


def test_loader_carries_groups_and_the_cpu_item_path_is_the_rule(tmp_path):
    import speech_imagery_eeg_amd  # noqa: F401
    from data_provider.data_factory import data_provider, ordered_loader
    from data_provider.eeg_npy import collate_raw_group, per_sample_standardise
    from utils.eeg_filter import filterbank_numpy
    s = S()
    X, y, subj = write_shards(str(tmp_path))
    M = np.random.RandomState(0).randn(3, 4, 6)
    np.save(tmp_path / "m.npy", M)
    labels = np.unique(subj)
    dense = np.searchsorted(labels, subj)
    seen = {}
    for flag in ("train", "val", "test"):
        ds, loader = data_provider(_ns(tmp_path, device_standardise=True, eeg_spatial=f"ref=car,matrix={tmp_path / 'm.npy'}"), flag)
        assert ds.enc_in == 4 and ds.groups == 3 and ds.spatial.Cs == 4 and np.array_equal(ds.spatial.labels, labels)
        assert np.array_equal(ds.group, dense) and ds.group.dtype == np.int32        # one dense mapping over the whole file
        assert loader.collate_fn is collate_raw_group and loader.eeg_chain.names == ["spatial"] and loader.eeg_chain.stages[0] is ds.spatial
        assert ordered_loader(loader).eeg_chain is loader.eeg_chain
        xb, yb, gid = next(iter(ordered_loader(loader)))
        n = min(8, len(ds))
        assert xb.shape == (n, 6, 64) and gid.dtype == torch.int32 and gid.tolist() == dense[ds.idx[:n]].tolist()
        seen[flag] = set(ds.idx.tolist())
    assert sum(len(v) for v in seen.values()) == 24 == len(set().union(*seen.values()))
    # the CPU item path: the fp32 form of the rule, then what the items were before
    W0 = s.compose("ref=car", 6, M)
    for pre in (None, "band=8:30,taps=21"):
        kw = {} if pre is None else dict(eeg_preprocess=pre)
        ds, loader = data_provider(_ns(tmp_path, device_standardise=False, eeg_spatial=f"ref=car,matrix={tmp_path / 'm.npy'}", **kw),
                                   "train")
        assert loader.eeg_chain is None and ds.enc_in == 4
        for i in (0, 5):
            j = ds.idx[i]
            v = s.spatial_numpy(X[j], W0[dense[j]].astype(np.float32), dtype=np.float32)
            if pre is None:
                want = per_sample_standardise(v).T
            else:
                p = ds.pre
                want = filterbank_numpy(v, p.taps2d.astype(np.float32), None, p.q, p.edge, p.Cout, p.Tout).astype(np.float32)
            got = ds[i][0]
            assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
        xb, yb, mask = next(iter(loader))
        assert xb.shape == (8, 64, 4) and mask.shape == (8, 64)
    # with fit, --target_channels counts virtual channels: enc_in is Cs before --eeg_preprocess resolves against it
    ds, _ = data_provider(_ns(tmp_path, device_standardise=False, eeg_spatial=f"matrix={tmp_path / 'm.npy'}",
                              eeg_preprocess="decimate=2,fit", target_channels=5, target_timepoints=30), "train")
    assert (ds.enc_in, ds.seq_len, ds.pre.Cout) == (5, 30, 5) and ds[0][0].shape == (30, 5) and not ds[0][0][:, 4].any()


def test_groups_without_the_file_with_a_wrong_matrix_and_without_need(tmp_path):
    import speech_imagery_eeg_amd  # noqa: F401
    from data_provider.eeg_chain import EEGChain
    from data_provider.eeg_npy import EEGNpyDataset
    write_shards(str(tmp_path))
    ds = EEGNpyDataset(str(tmp_path), flag="train", chain=EEGChain(spatial="ref=car"))        # no groups needed: the file is not read
    assert ds.groups == 1 and not ds.group.any() and ds.spatial.W.shape == (1, 6, 6)
    np.save(tmp_path / "two.npy", np.zeros((2, 4, 6)))
    with pytest.raises(ValueError, match="holds 2 groups, the shards 3"):
        EEGNpyDataset(str(tmp_path), flag="train", chain=EEGChain(spatial=f"matrix={tmp_path / 'two.npy'}"))
    np.save(tmp_path / "subject.npy", np.zeros(24))                           # float ids
    with pytest.raises(ValueError, match="integer subject ids"):
        EEGNpyDataset(str(tmp_path), flag="train", chain=EEGChain(spatial="align=euclid"))
    os.remove(tmp_path / "subject.npy")
    ds = EEGNpyDataset(str(tmp_path), flag="val", chain=EEGChain(spatial="align=euclid"))     # only the training split speaks
    assert ds.groups == 1 and not ds.group.any()
    said = []
    again = EEGChain(spatial="align=euclid").resolve(6, 64, str(tmp_path), 24, notice=said.append)
    assert again.stage("spatial").groups == 1 and not again.group.any() and len(said) == 1 and "one group" in said[0]


def test_experiment_fits_saves_and_builds_for_cs_channels_on_the_cpu(tmp_path, monkeypatch):
    """The harness on a CPU device (numpy path): the alignment is fitted from the training split before the model is built, all three
    splits get it, eeg_spatial.npz records it, and a second run writes the same bytes."""
    import speech_imagery_eeg_amd  # noqa: F401
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # the CPU-device harness, whatever the machine has
    import run as driver
    from exp.experiment_classification import Experiment
    s = S()
    X, y, subj = write_shards(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    files = []
    for _ in range(2):
        args = driver.get_args(["--model", "SBM", "--data", "EEG3", "--data_root", str(tmp_path), "--dataset", "chisco_npy",
                                "--batch_size", "8", "--seed", "0", "--num_workers", "0", "--eeg_spatial", "ref=car,align=euclid"])
        driver.set_seed(0)
        exp = Experiment(args)
        assert args.enc_in == 6
        st = exp.train_data.spatial
        assert st.fitted and st.W.shape == (3, 6, 6) and exp.val_data.spatial.W is st.W and exp.test_data.spatial.W is st.W
        f = np.load(os.path.join(exp.checkpoint_dir, s.FILE_NAME))
        assert f["W"].tobytes() == st.W.tobytes() and f["labels"].tolist() == sorted(set(subj.tolist()))
        assert s.parse_eeg_spatial(str(f["spec"])) == st.spec and bool(f["fitted"])
        files.append(f["W"].tobytes())
        # the items of every split are whitened per subject: the aligned training trials have covariance H
        tr = exp.train_data
        batches = list(tr.raw_batches(8))
        want = s.fit_alignment(batches, st.W0, 3, 1e-6)
        assert want.tobytes() == st.W.tobytes()
    assert files[0] == files[1]


# --------------------------------------------------------------------------------------------------------------------- ABI
NAMES = ("ign_eeg_spatial_nct", "ign_eeg_gram_ws_bytes", "ign_eeg_gram_nct")
E_ARG, E_TOOBIG = -1001, -1003


def _header_params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/ign_abi.h"
    return [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")]


def test_the_three_symbols_are_in_the_header_and_in_the_table():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    s = S()
    want = {"ign_eeg_spatial_nct": ["x_nct", "w_gsc", "gid", "out_nst", "B", "Cin", "T", "Cs", "G", "stream"],
            "ign_eeg_gram_ws_bytes": ["B", "C", "T", "G"],
            "ign_eeg_gram_nct": ["x_nct", "gid", "gram_gcc", "count_g", "ws", "B", "C", "T", "G", "stream"]}
    for name in NAMES:
        assert _header_params(name) == want[name]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(want[name])
    assert _lib.SIGNATURES["ign_eeg_gram_ws_bytes"][0] is ctypes.c_size_t
    hdr = open(os.path.join(ROOT, "include", "ign_abi.h")).read()
    limits = {k: int(v) for k, v in re.findall(r"#define\s+(IGN_EEG_SPATIAL_MAX_\w+)\s+(\d+)", hdr)}
    assert limits == {"IGN_EEG_SPATIAL_MAX_CHANNELS": s.MAX_CHANNELS, "IGN_EEG_SPATIAL_MAX_GROUPS": s.MAX_GROUPS}
    assert s.MAX_CHANNELS >= 512 and s.MAX_GROUPS >= 64


def _p(v):
    return ctypes.c_void_p(v)


def _lib_or_skip():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so is not built")
    return _lib.lib()


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(x=None), E_ARG, b"null pointer"), (dict(w=None), E_ARG, b"null pointer"), (dict(out=None), E_ARG, b"null pointer"),
    (dict(B=0), E_ARG, b"non-positive"), (dict(Cin=0), E_ARG, b"non-positive"), (dict(T=-1), E_ARG, b"non-positive"),
    (dict(Cs=0), E_ARG, b"non-positive"), (dict(G=0), E_ARG, b"non-positive"),
    (dict(B=65536), E_TOOBIG, b"65535"), (dict(Cin=513), E_TOOBIG, b"Cin=513"), (dict(Cs=513), E_TOOBIG, b"Cs=513"),
    (dict(G=65), E_TOOBIG, b"G=65"),
])
def test_apply_refusals_return_before_any_launch(kw, rc, msg):
    L = _lib_or_skip()
    a = dict(x=_p(16), w=_p(32), gid=None, out=_p(48), B=2, Cin=4, T=60, Cs=4, G=1, stream=None)
    a.update(kw)
    assert L.ign_eeg_spatial_nct(*a.values()) == rc
    assert msg in L.ign_last_error() and b"ign_eeg_spatial_nct" in L.ign_last_error()


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(x=None), E_ARG, b"null pointer"), (dict(gram=None), E_ARG, b"null pointer"), (dict(count=None), E_ARG, b"null pointer"),
    (dict(ws=None), E_ARG, b"null pointer"), (dict(B=0), E_ARG, b"non-positive"), (dict(C=0), E_ARG, b"non-positive"),
    (dict(T=0), E_ARG, b"non-positive"), (dict(G=-2), E_ARG, b"non-positive"),
    (dict(B=65536), E_TOOBIG, b"65535"), (dict(C=513), E_TOOBIG, b"C=513"), (dict(G=65), E_TOOBIG, b"G=65"),
])
def test_gram_refusals_return_before_any_launch(kw, rc, msg):
    L = _lib_or_skip()
    a = dict(x=_p(16), gid=None, gram=_p(32), count=_p(48), ws=_p(64), B=2, C=4, T=60, G=1, stream=None)
    a.update(kw)
    assert L.ign_eeg_gram_nct(*a.values()) == rc
    assert msg in L.ign_last_error() and b"ign_eeg_gram_nct" in L.ign_last_error()
    dims = [a[k] for k in ("B", "C", "T", "G")]
    if set(kw) & {"B", "C", "T", "G"}:
        assert L.ign_eeg_gram_ws_bytes(*dims) == 0
    else:
        assert L.ign_eeg_gram_ws_bytes(*dims) == (2 * 4 + 2 * 4 * 4) * 4
