"""GPU side of the spatial filter stage: ops.eeg_spatial (ign_eeg_spatial_nct) and ops.eeg_gram (ign_eeg_gram_nct) against the float64
rules with a-priori bounds (tests/eeg_spatial_cases.py), their structural guarantees (every element written, fixed order, a sample
does not depend on its batch, out-of-range groups), the refusals through ops, then the prefetcher, the fit and the harness on
temporary shards with subject ids.  The host side is tests/test_eeg_spatial_host.py."""
import os

import numpy as np
import pytest
import torch

from eeg_spatial_cases import APPLY_CASES, GRAM_CASES, S, apply_case, check_apply, gram_case, identity_expectation, write_shards

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


def _nan(*shape, dev):
    return torch.full(shape, float("nan"), device=dev)


# ------------------------------------------------------------------------------------------------------------------- apply
@pytest.mark.parametrize("label", list(APPLY_CASES))
def test_apply_meets_both_bounds_and_writes_every_element(label):
    ops, dev = _ops(), _dev()
    k = apply_case(label)
    B, Cin, T, Cs, G, _, _ = APPLY_CASES[label]
    out = _nan(B, Cs, T, dev=dev)
    y = ops.eeg_spatial(_t(k["x"], dev), _t(k["W"], dev), _t(k["gid"], dev), out=out)
    assert y is out and y.shape == (B, Cs, T) and y.dtype == torch.float32
    got = y.cpu().numpy()
    assert np.isfinite(got).all()                                            # every element written, none left NaN
    check_apply(label, got)
    new = ops.eeg_spatial(_t(k["x"], dev), _t(k["W"], dev), _t(k["gid"], dev))          # without out=
    assert torch.equal(new, y)


@pytest.mark.parametrize("label", list(APPLY_CASES))
def test_identity_gives_x_bit_for_bit(label):
    """W = I: x itself on every element whose pivot subtraction is exact in fp32 (all of them in four of the six cases; all but
    117 / 1102 elements of 2 / 3 rows in E_unused_group / F_real_row, rows whose offset is below their signal), and the rule's
    fl(fl(x - p) + p) on every element: the chain adds exact zeros, the k padding included."""
    ops, dev = _ops(), _dev()
    x = apply_case(label)["x"]
    want, exact = identity_expectation(x)
    y = ops.eeg_spatial(_t(x, dev), torch.eye(x.shape[1], device=dev)).cpu().numpy()
    assert np.array_equal(y, want)
    assert np.array_equal(y[exact], x[exact]) and exact.mean() > 0.99
    if label not in ("E_unused_group", "F_real_row"):
        assert exact.all() and np.array_equal(y, x)


def test_two_calls_agree_and_a_sample_does_not_depend_on_its_batch():
    ops, dev = _ops(), _dev()
    k = apply_case("C_tile_crossing")
    x, W, gid = _t(k["x"], dev), _t(k["W"], dev), _t(k["gid"], dev)
    a, b = ops.eeg_spatial(x, W, gid), ops.eeg_spatial(x, W, gid)
    assert torch.equal(a, b)
    for i in range(x.shape[0]):                                               # every sample alone: the bits it has in the batch
        assert torch.equal(ops.eeg_spatial(x[i:i + 1], W, gid[i:i + 1]), a[i:i + 1]), i
        assert torch.equal(ops.eeg_spatial(x[i:i + 1], W[int(gid[i])]), a[i:i + 1]), i             # a 2-D W is one group
    rev = ops.eeg_spatial(x.flip(0).contiguous(), W, gid.flip(0).contiguous())
    assert torch.equal(rev.flip(0), a)
    wide = torch.zeros(3, 33, 260, device=dev)                               # a non-contiguous x is copied, as eeg_filterbank does
    wide[:, :, ::2] = x
    view = wide[:, :, ::2]
    assert not view.is_contiguous() and torch.equal(ops.eeg_spatial(view, W, gid), a)
    assert torch.equal(ops.eeg_spatial(x, W.transpose(1, 2).contiguous().transpose(1, 2), gid), a)


@pytest.mark.parametrize("bad", [2, -1, 1 << 30])
def test_a_group_outside_the_table_gives_zeros_there_and_nothing_else_moves(bad):
    ops, dev = _ops(), _dev()
    k = apply_case("C_tile_crossing")
    x, W = _t(k["x"], dev), _t(k["W"], dev)
    ok = ops.eeg_spatial(x, W, _t(k["gid"], dev))
    gid = k["gid"].copy()
    gid[1] = bad
    y = ops.eeg_spatial(x, W, _t(gid, dev), out=_nan(3, 7, 130, dev=dev))
    assert bool((y[1] == 0).all()) and torch.equal(y[0], ok[0]) and torch.equal(y[2], ok[2])


# -------------------------------------------------------------------------------------------------------------------- gram
@pytest.mark.parametrize("label", list(GRAM_CASES))
def test_gram_meets_its_bound_is_symmetric_and_repeatable(label):
    ops, dev = _ops(), _dev()
    k = gram_case(label)
    B, C, T, G, _ = GRAM_CASES[label]
    x, gid = _t(k["x"], dev), _t(k["gid"], dev)
    gram = _nan(G, C, C, dev=dev)
    count = torch.full((G,), -7, device=dev, dtype=torch.int32)
    g2, c2 = ops.eeg_gram(x, gid, G, out=(gram, count))
    assert g2 is gram and c2 is count
    got = gram.double().cpu().numpy()
    assert np.isfinite(got).all() and count.cpu().tolist() == k["count"].tolist()
    err = np.abs(got - k["gram64"])
    ratio = float((err / np.maximum(k["bound"], 1e-300))[k["bound"] > 0].max())
    print(f"eeg_gram {label}: error / bound = {ratio:.4f}")
    assert (err <= k["bound"]).all(), ratio
    assert torch.equal(gram, gram.transpose(1, 2))                           # bit for bit
    for g in range(G):
        if k["count"][g] == 0:
            assert not bool(gram[g].any())                                    # an empty group: exact zeros
    again, cagain = ops.eeg_gram(x, gid, G)
    assert torch.equal(again, gram) and torch.equal(cagain, count)
    if gid is not None:                                                       # a group's Gram is the Gram of its samples alone
        for g in range(G):
            sel = torch.nonzero(gid == g).flatten()
            if len(sel):
                alone, n = ops.eeg_gram(x[sel].contiguous(), None, 1)
                assert torch.equal(alone[0], gram[g]) and int(n[0]) == len(sel)


def test_gram_ignores_samples_outside_the_table():
    ops, dev = _ops(), _dev()
    k = gram_case("A_small")
    x = _t(k["x"], dev)
    full, _ = ops.eeg_gram(x, _t(k["gid"], dev), 2)
    gram, count = ops.eeg_gram(x, _t(np.asarray([1, 5, -1], dtype=np.int32), dev), 2)
    alone, _ = ops.eeg_gram(x[:1], None, 1)
    assert count.tolist() == [0, 1] and not bool(gram[0].any()) and torch.equal(gram[1], alone[0])
    assert not torch.equal(gram[1], full[1])


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_through_ops_leave_the_output_untouched():
    ops, dev = _ops(), _dev()
    from ign_hip._lib import IgnError
    s = S()
    z = lambda *shape: torch.zeros(*shape, device=dev)                        # noqa: E731
    # IGN_E_ARG / IGN_E_TOOBIG of the launcher, each with an output that must stay as it was
    apply = [
        (z(0, 2, 8), z(1, 2, 2), "null pointer|non-positive"), (z(1, 2, 0), z(1, 2, 2), "null pointer|non-positive"),
        (z(1, 2, 8), z(1, 0, 2), "null pointer|non-positive"), (z(1, 2, 8), z(0, 2, 2), "null pointer|non-positive"),
        (z(1, s.MAX_CHANNELS + 1, 4), z(1, 2, s.MAX_CHANNELS + 1), "Cin=513"), (z(1, 2, 4), z(1, s.MAX_CHANNELS + 1, 2), "Cs=513"),
        (z(1, 2, 4), z(s.MAX_GROUPS + 1, 2, 2), "G=65"),
    ]
    for x, W, msg in apply:
        out = _nan(x.shape[0], W.shape[1], x.shape[2], dev=dev)
        with pytest.raises(IgnError, match=msg):
            ops.eeg_spatial(x, W, out=out)
        assert bool(torch.isnan(out).all())
    big = torch.empty(65536, 1, 1, device=dev)
    out = _nan(65536, 1, 1, dev=dev)
    with pytest.raises(IgnError, match="65535"):
        ops.eeg_spatial(big, z(1, 1, 1), out=out)
    assert bool(torch.isnan(out).all())
    for x, G, msg in [(z(0, 2, 8), 1, "null pointer|non-positive"), (z(2, 2, 0), 1, "null pointer|non-positive"),
                      (z(2, 2, 8), 0, "null pointer|non-positive"), (z(1, s.MAX_CHANNELS + 1, 2), 1, "C=513"),
                      (z(2, 2, 8), s.MAX_GROUPS + 1, "G=65"), (big, 1, "65535")]:
        gram, count = _nan(max(G, 0), x.shape[1], x.shape[1], dev=dev), torch.full((max(G, 0),), -7, device=dev, dtype=torch.int32)
        with pytest.raises(IgnError, match=msg):
            ops.eeg_gram(x, None, G, out=(gram, count))
        assert bool(torch.isnan(gram).all()) and bool((count == -7).all())
    # the shape and dtype checks beside eeg_filterbank's
    x = z(2, 3, 8)
    with pytest.raises(IgnError, match="expected x"):
        ops.eeg_spatial(x[0], z(3, 3))
    with pytest.raises(IgnError, match="expected x"):
        ops.eeg_spatial(x, z(3))
    with pytest.raises(IgnError, match="input channels"):
        ops.eeg_spatial(x, z(3, 4))
    with pytest.raises(IgnError, match="gid must be"):
        ops.eeg_spatial(x, z(2, 3, 3), torch.zeros(2, device=dev, dtype=torch.int64))
    with pytest.raises(IgnError, match="gid must be"):
        ops.eeg_spatial(x, z(2, 3, 3), torch.zeros(3, device=dev, dtype=torch.int32))
    with pytest.raises(IgnError, match="gid must be"):
        ops.eeg_gram(x, torch.zeros(2, dtype=torch.int32), 2)
    with pytest.raises(IgnError, match="out must be"):
        ops.eeg_spatial(x, z(3, 3), out=z(2, 3, 9))
    with pytest.raises(IgnError, match="float32"):
        ops.eeg_spatial(x.double(), z(3, 3))
    with pytest.raises(IgnError, match="no CPU fallback"):
        ops.eeg_spatial(x.cpu(), z(3, 3))
    with pytest.raises(IgnError, match="expected x"):
        ops.eeg_gram(x[0])


# ------------------------------------------------------------------------------------------------- prefetcher, fit, harness
def _fit_on(ds, dev, spec_W0, groups, rtol=1e-6):
    """fit_alignment over the training split's raw trials on `dev` (None: the numpy path)"""
    s = S()
    batches = list(ds.raw_batches(8))
    if dev is not None:
        batches = [(torch.from_numpy(x).to(dev), None, torch.from_numpy(g).to(dev)) for x, _, g in batches]
    return s.fit_alignment(batches, spec_W0, groups, rtol, notice=None)


@pytest.mark.parametrize("pre", [None, "band=8:30,taps=41"], ids=["standardise", "bandpass"])
@pytest.mark.parametrize("spec", ["ref=car", "ref=car,align=euclid"])
def test_prefetcher_with_the_composed_transform_equals_the_cpu_loader_path(tmp_path, spec, pre):
    """The raw device path (spatial launch, then the standardisation or the band-pass transform) against the CPU loader path (the
    rule's fp32 restatement per item, then the numpy rules), judged like
    test_prefetcher_with_the_preprocess_transform_equals_the_cpu_loader_path: conftest.parity, element-wise at the project's
    tolerance, with the float64 form of the whole path beside it.  taps=41 because the default for an 8 Hz edge, 207 taps, reflects
    103 samples and the rows have 64.  With align=, W is fitted on the device and must equal the numpy fit to 1e-5 max|W|."""
    from conftest import NORTH_STAR_TOL, parity
    dev, s = _dev(), S()
    _ops()
    from data_provider.device_prefetch import DevicePrefetcher
    from data_provider.eeg_chain import EEGChain
    from data_provider.eeg_npy import EEGNpyDataset, collate_raw_group, per_sample_standardise
    from data_provider.uea import collate_fn
    from utils.eeg_filter import filterbank_numpy, pad_time
    X, y, subj = write_shards(str(tmp_path))
    kw = dict(chain=EEGChain(spatial=spec, preprocess=pre))
    cpu = EEGNpyDataset(str(tmp_path), flag="train", **kw)
    raw = EEGNpyDataset(str(tmp_path), flag="train", raw=True, **kw)
    assert raw.enc_in == cpu.enc_in == 6 and raw.groups == (3 if "align" in spec else 1)
    if "align" in spec:
        W = _fit_on(raw, dev, raw.spatial.W0, 3)
        Wn = _fit_on(raw, None, raw.spatial.W0, 3)
        assert W.shape == (3, 6, 6) and float(np.abs(W - Wn).max()) <= 1e-5 * float(np.abs(Wn).max())
        assert _fit_on(raw, dev, raw.spatial.W0, 3).tobytes() == W.tobytes()
        cpu.spatial.W = raw.spatial.W = W
    W = raw.spatial.W
    want = list(torch.utils.data.DataLoader(cpu, batch_size=8, shuffle=False, collate_fn=lambda b: collate_fn(b, max_len=cpu.seq_len)))
    loader = torch.utils.data.DataLoader(raw, batch_size=8, shuffle=False, collate_fn=collate_raw_group, pin_memory=True)
    assert raw.chain.names == ["spatial"] + ([] if pre is None else ["preprocess"])
    got = list(DevicePrefetcher(loader, dev, transform=raw.chain.device_transform(dev)))           # built behind the fit: it reads W
    assert len(got) == len(want) == 3
    for i, ((a, b, m), (c, d, n)) in enumerate(zip(got, want)):
        j = raw.idx[8 * i:8 * i + 8]
        v64 = s.spatial_numpy(X[j], W, raw.group[j])
        if pre is None:
            f64 = np.swapaxes(per_sample_standardise(v64), 1, 2)
        else:
            p = raw.pre
            f64, _ = pad_time(filterbank_numpy(v64, p.taps2d.astype(np.float32), None, p.q, p.edge, p.Cout, p.Tout), p.Tout)
        assert a.is_cuda and a.shape == c.shape == f64.shape == (len(j), 64, 6)
        # The stage's output is an fp32 number that carries the row's offset (|P| up to 3e4 uV: half an ulp is 1e-3 uV, 2e-4 of a
        # 5 uV standard deviation), and the fp32 statistics behind it sum such numbers: the restatement itself is 7e-5 to 3.4e-4
        # of 1 + |ref| away from float64 on these shards (profiles/eeg_spatial.json, cpu_emulation).  So the bound is the
        # restatement's own distance, computed here on the CPU, never the kernel's: the kernel may be as far from float64 as the
        # restatement is, to the margin of 2 that two independent fp32 orders of the same sums warrant, and then the two are at most
        # the sum of both distances apart.
        e_ref = float((np.abs(c.double().numpy() - f64) / (1.0 + np.abs(f64))).max())
        tol = max(NORTH_STAR_TOL, 2.0 * e_ref)
        e_hip = float((np.abs(a.double().cpu().numpy() - f64) / (1.0 + np.abs(f64))).max())
        print(f"eeg_spatial prefetcher {spec} {pre} batch {i}: restatement vs float64 {e_ref:.3e}, kernel vs float64 {e_hip:.3e}")
        assert e_hip <= tol, (e_hip, e_ref)
        parity(f"eeg_spatial prefetcher {spec} {pre} batch {i}", a, c, tol=tol, kind="elem", f64=f64,
               ref_is="CPU loader path: numpy float32 restatement of the spatial rule, then the numpy rules; tol = twice its own "
                      "distance from float64")
        assert torch.equal(b.cpu(), d) and torch.equal(m.cpu().bool(), n.bool())


def test_a_run_without_the_flag_launches_neither_kernel(tmp_path):
    dev = _dev()
    _ops()
    from ign_hip import _lib
    from data_provider.device_prefetch import DevicePrefetcher, standardise_raw_batch
    from data_provider.eeg_chain import EEGChain
    from data_provider.eeg_npy import EEGNpyDataset, collate_raw, collate_raw_group
    write_shards(str(tmp_path))
    _lib.timing_enable(True)
    try:
        raw = EEGNpyDataset(str(tmp_path), flag="train", raw=True)
        loader = torch.utils.data.DataLoader(raw, batch_size=8, shuffle=False, collate_fn=collate_raw)
        plain = list(DevicePrefetcher(loader, dev, transform=standardise_raw_batch))
        torch.cuda.synchronize()
        assert _lib.timing_read("eeg_spatial")[1] == 0 and _lib.timing_read("eeg_gram")[1] == 0
        on = EEGNpyDataset(str(tmp_path), flag="train", raw=True, chain=EEGChain(spatial="matrix=" + _identity(tmp_path)))
        loader = torch.utils.data.DataLoader(on, batch_size=8, shuffle=False, collate_fn=collate_raw_group)
        same = list(DevicePrefetcher(loader, dev, transform=on.chain.device_transform(dev)))
        torch.cuda.synchronize()
        assert _lib.timing_read("eeg_spatial")[1] == 3 and _lib.timing_read("eeg_gram")[1] == 0
    finally:
        _lib.timing_enable(False)
    for (a, _, ma), (b, _, mb) in zip(plain, same):                           # the identity in front: the same batches to fp32 rounding
        assert a.shape == b.shape and torch.equal(ma, mb) and float((a - b).abs().max()) < 1e-3


def _identity(tmp_path):
    np.save(tmp_path / "eye.npy", np.eye(6))
    return str(tmp_path / "eye.npy")


def test_harness_trains_with_the_alignment_and_records_it(tmp_path, monkeypatch):
    """Experiment on shards with subject.npy under --eeg_spatial ref=car,align=euclid: the alignment is fitted on the device before
    the model is built (for Cs channels), three steps of an SBM give finite losses, eeg_spatial.npz is written, and a second run
    writes the same bytes of W."""
    _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    import run as driver
    from exp.experiment_classification import Experiment
    s = S()
    M = np.random.RandomState(0).randn(5, 6)
    X, y, subj = write_shards(str(tmp_path))
    np.save(tmp_path / "m.npy", M)
    monkeypatch.chdir(tmp_path)
    seen = []
    for _ in range(2):
        args = driver.get_args(["--model", "SBM", "--data", "EEG3", "--data_root", str(tmp_path), "--dataset", "chisco_npy",
                                "--train_epochs", "1", "--batch_size", "8", "--seed", "0", "--num_workers", "0",
                                "--eeg_spatial", f"ref=car,align=euclid,matrix={tmp_path / 'm.npy'}"])
        driver.set_seed(0)
        exp = Experiment(args)
        assert args.enc_in == 5 and args.seq_len == 64                      # the model was built for Cs channels
        st = exp.train_data.spatial
        assert st.fitted and st.W.shape == (3, 5, 6) and st.W.dtype == np.float32
        per_step, step = exp.train_one_epoch(0, 0)
        losses = [float(v) for v in per_step]
        assert step == 3 == len(losses) and all(np.isfinite(v) for v in losses), losses
        f = np.load(os.path.join(exp.checkpoint_dir, s.FILE_NAME))
        assert f["W"].tobytes() == st.W.tobytes() and f["labels"].tolist() == sorted(set(subj.tolist())) and bool(f["fitted"])
        seen.append((f["W"].tobytes(), losses))
        xb, _, mask = next(iter(exp.val_loader))
        assert xb.shape[1:] == (64, 5) and mask.shape[1] == 64
    assert seen[0][0] == seen[1][0]
    # behind the fit every subject's training trials have the identity as the mean covariance of their 5 virtual channels
    # (to 1e-2: a W that was not fitted, or fitted for another subject, is wrong by O(1); the device fit's own distance from the
    # float64 fit is the subject of the prefetcher test)
    trials, groups = zip(*[(xb, gb) for xb, _, gb in exp.train_data.raw_batches(8)])
    trials, groups = np.concatenate(trials), np.concatenate(groups)
    for g in range(3):
        z = s.spatial_numpy(trials[groups == g], st.W[g])
        z = z - z.mean(axis=-1, keepdims=True)
        assert np.allclose(np.einsum('bit,bjt->ij', z, z) / (len(z) * 64), np.eye(5), atol=1e-2), g
