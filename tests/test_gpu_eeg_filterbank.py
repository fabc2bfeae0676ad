"""GPU parity of the EEG filter bank: ops.eeg_filterbank (ign_eeg_filterbank_nct_to_btc) against the rule restated in numpy
(utils/eeg_filter.py:filterbank_numpy) -- float64 on the fp32 input and fp32-rounded taps as the oracle, a plain float32 restatement
beside it -- block by block against ops.eeg_preprocess bit for bit, then the prefetcher and the harness on the bank.  The case table
and its references are tests/eeg_filterbank_cases.py; the host side is tests/test_eeg_filterbank_host.py."""
import numpy as np
import pytest
import torch

from eeg_filterbank_cases import CASES, bank_taps, case, recordings

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _mods():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    from utils import eeg_filter
    return ops, eeg_filter


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check(label, k, edge="reflect"):
    """one call of the op on case `k` against its references, plus the structural assertions of every case"""
    from conftest import parity
    ops, F = _mods()
    dev = _dev()
    x, nb, Cout, Tout, Tv, Cv = k["x"], k["nb"], k["Cout"], k["Tout"], k["Tv"], k["Cv"]
    out, mask = ops.eeg_filterbank(_t(x, dev), _t(k["H"], dev), _t(k["G"], dev), decimate=k["q"], edge=edge, channels=Cout,
                                   timepoints=Tout)
    assert out.shape == (x.shape[0], Tout, nb * Cout) and out.dtype == torch.float32
    assert mask.dtype == torch.bool and mask.shape == (x.shape[0], Tout)
    assert np.array_equal(mask.cpu().numpy(), np.broadcast_to(k["mask"], mask.shape))
    parity(f"eeg_filterbank {label}", out, k["ref32"], kind="elem", f64=k["ref64"], ref_is="numpy float32 restatement of the rule")
    o = out.cpu()
    assert bool(torch.isfinite(o).all())
    assert bool((o[:, Tv:] == 0).all())                                      # padding rows: exact zeros
    blocks = o.view(x.shape[0], Tout, nb, Cout)
    assert bool((blocks[..., Cv:] == 0).all())                               # the padded electrodes of EVERY block
    v = blocks[:, :Tv, :, :Cv].double()
    assert float(v.mean(dim=1).abs().max()) < 1e-3                           # the statistics are those of the valid part
    assert float((v.std(dim=1, unbiased=True) - 1).abs().max()) < 1e-3
    return out


@pytest.mark.parametrize("label", list(CASES))
@pytest.mark.parametrize("envelope", [False, True], ids=["plain", "envelope"])
def test_kernel_matches_the_rule(label, envelope):
    _check(f"{label} {'envelope' if envelope else 'plain'}", case(label, envelope))


def test_kernel_matches_the_rule_with_zero_extension():
    _check("B_crop_pad plain zero", case("B_crop_pad", False, "zero"), edge="zero")


@pytest.mark.parametrize("label", ["A_one_band", "C_tile_crossing", "E_two_sweeps"])
def test_block_j_is_the_one_band_op_bit_for_bit(label):
    """Without quad, band j's tap walk, statistics and output line do not depend on the other bands, so block j is the bank of one that
    ops.eeg_preprocess runs with H[j]: the same operations in the same order, the same bits.  A_one_band is nb = 1: the whole output."""
    ops, F = _mods()
    dev = _dev()
    k = case(label, False)
    x, H, Cout = _t(k["x"], dev), _t(k["H"], dev), k["Cout"]
    kw = dict(decimate=k["q"], edge="reflect", channels=Cout, timepoints=k["Tout"])
    out, mask = ops.eeg_filterbank(x, H, **kw)
    for j in range(k["nb"]):
        want, want_mask = ops.eeg_preprocess(x, H[j], **kw)
        assert torch.equal(out[:, :, j * Cout:(j + 1) * Cout], want), (label, j)
        assert torch.equal(mask, want_mask)
    if k["nb"] == 1:
        assert torch.equal(out, ops.eeg_preprocess(x, H[0], **kw)[0])
        for edge in ("reflect", "zero"):                                     # nb = 1 at the defaults, both edge modes
            assert torch.equal(ops.eeg_filterbank(x, H, edge=edge)[0], ops.eeg_preprocess(x, H[0], edge=edge)[0]), edge


def test_two_calls_are_bit_identical_and_strides_do_not_matter():
    ops, F = _mods()
    dev = _dev()
    x = torch.from_numpy(recordings(3, 37, 301)).to(dev)
    H, G = (_t(a, dev) for a in bank_taps(((8, 13), (13, 30), (30, 45)), 101))
    kw = dict(decimate=2, channels=40, timepoints=128)
    wide = torch.zeros(3, 37, 602, device=dev)
    wide[:, :, ::2] = x
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    for quad in (None, G):
        a, ma = ops.eeg_filterbank(x, H, quad, **kw)
        b, mb = ops.eeg_filterbank(x, H, quad, **kw)
        assert a.shape == (3, 128, 120) and torch.equal(a, b) and torch.equal(ma, mb)
        c, _ = ops.eeg_filterbank(view, H, quad, **kw)
        assert torch.equal(a, c)
        Hw = torch.zeros(3, 202, device=dev)
        Hw[:, ::2] = H
        d, _ = ops.eeg_filterbank(x, Hw[:, ::2], quad, **kw)                 # strided taps too
        assert torch.equal(a, d)
    assert not torch.equal(ops.eeg_filterbank(x, H, None, **kw)[0], ops.eeg_filterbank(x, H, G, **kw)[0])


def test_ops_refusals_on_the_device():
    ops, F = _mods()
    from ign_hip._lib import IgnError
    dev = _dev()
    x = torch.zeros(1, 2, 40, device=dev)
    with pytest.raises(IgnError, match="bands outside 1..8"):
        ops.eeg_filterbank(x, torch.ones(9, 5, device=dev))
    with pytest.raises(IgnError, match="IGN_EDGE_ZERO"):
        ops.eeg_filterbank(x, torch.ones(2, 5, device=dev), torch.ones(2, 5, device=dev), edge="zero")
    with pytest.raises(IgnError, match="M=1"):
        ops.eeg_filterbank(x, torch.ones(2, 1, device=dev), torch.ones(2, 1, device=dev))
    with pytest.raises(IgnError, match="shape of taps"):
        ops.eeg_filterbank(x, torch.ones(2, 5, device=dev), torch.ones(2, 7, device=dev))
    with pytest.raises(IgnError, match=r"taps \(nb,M\)"):
        ops.eeg_filterbank(x, torch.ones(5, device=dev))
    with pytest.raises(IgnError, match="odd count"):
        ops.eeg_filterbank(x, torch.ones(2, 4, device=dev))
    with pytest.raises(IgnError, match="reflect extension"):
        ops.eeg_filterbank(x, torch.ones(2, 81, device=dev))
    with pytest.raises(ValueError):
        ops.eeg_filterbank(x, torch.ones(2, 5, device=dev), edge="wrap")


@pytest.mark.parametrize("envelope", [False, True], ids=["plain", "envelope"])
def test_prefetcher_with_the_bank_transform_equals_the_cpu_loader_path(tmp_path, envelope):
    dev = _dev()
    ops, F = _mods()
    from data_provider.device_prefetch import DevicePrefetcher
    from data_provider.eeg_chain import EEGChain
    from data_provider.eeg_npy import EEGNpyDataset3Class, collate_raw
    from data_provider.uea import collate_fn
    rng = np.random.RandomState(1)
    X = (rng.randn(50, 12, 200) * 30 + 500).astype(np.float32)
    np.save(tmp_path / "X.npy", X)
    np.save(tmp_path / "y.npy", rng.randint(0, 39, size=50))
    spec = "bank=8:13+13:30+30:45,decimate=2,fit" + (",envelope" if envelope else "")
    kw = dict(chain=EEGChain(preprocess=spec, target_channels=8, target_timepoints=120))
    cpu = EEGNpyDataset3Class(str(tmp_path), flag="train", **kw)
    raw = EEGNpyDataset3Class(str(tmp_path), flag="train", raw=True, **kw)
    assert (raw.seq_len, raw.enc_in, raw.pre.Tv) == (120, 24, 100) and isinstance(raw.pre, F.ResolvedBank)
    want = list(torch.utils.data.DataLoader(cpu, batch_size=16, shuffle=False, collate_fn=lambda b: collate_fn(b, max_len=cpu.seq_len)))
    loader = torch.utils.data.DataLoader(raw, batch_size=16, shuffle=False, collate_fn=collate_raw, pin_memory=True)
    got = list(DevicePrefetcher(loader, dev, transform=raw.chain.device_transform(dev)))
    assert len(got) == len(want)
    for (a, b, m), (c, d, n) in zip(got, want):
        assert a.is_cuda and a.shape == c.shape == (a.shape[0], 120, 24)
        assert float((a.cpu() - c).abs().max()) < 1e-4                      # the bound of the one-band test of the same name
        assert torch.equal(b.cpu(), d) and torch.equal(m.cpu(), n)


def test_harness_trains_on_the_envelope_bank(tmp_path, monkeypatch):
    """Experiment on CHISCO-contract shards with bank=8:13+13:30,decimate=2,envelope: the model is built for 2 * 10 channels, two
    epochs give finite losses, and a second run from the same seed repeats them exactly.  taps=101 because the default for an
    8 Hz edge, 207 taps, reflects 103 samples and the rows have 100."""
    _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    import run as driver
    from exp.experiment_classification import Experiment
    rng = np.random.RandomState(2)
    y = rng.randint(0, 39, size=96)
    X = (rng.randn(96, 10, 100) * 20 + 300).astype(np.float32)
    t = np.arange(20) / 500.0
    X[:, 0, 10:30] += (y // 13)[:, None] * 40.0 * np.sin(2 * np.pi * 20.0 * t)[None, :]       # a class-dependent beta burst
    np.save(tmp_path / "X.npy", X)
    np.save(tmp_path / "y.npy", y)
    monkeypatch.chdir(tmp_path)
    losses = []
    for _ in range(2):
        args = driver.get_args(["--model", "InterpGN", "--dnn_type", "FCN", "--data", "EEG3", "--data_root", str(tmp_path),
                                "--dataset", "chisco_npy", "--train_epochs", "2", "--batch_size", "32", "--seed", "0", "--amp",
                                "--min_epochs", "5", "--num_workers", "0", "--eeg_preprocess", "bank=8:13+13:30,decimate=2,envelope,taps=101"])
        driver.set_seed(0)
        exp = Experiment(args)
        assert args.enc_in == 2 * 10 and args.seq_len == 50                 # the model is built for bands x electrodes
        run, step = [], 0
        for epoch in range(2):
            per_step, step = exp.train_one_epoch(epoch, step)
            run += [float(v) for v in per_step]
        run += [float(v) for v in exp.validation()]
        assert len(run) == 2 * len(exp.train_loader) + 2 and all(np.isfinite(v) for v in run), run
        losses.append(run)
    assert losses[0] == losses[1], losses
