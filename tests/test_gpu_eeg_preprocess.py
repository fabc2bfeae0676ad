"""GPU parity of --eeg_preprocess: ops.eeg_preprocess (ign_eeg_preprocess_nct_to_btc) against the rule restated in numpy
(utils/eeg_filter.py:preprocess_numpy) -- float64 on the fp32 input and fp32-rounded taps as the oracle, a plain float32 restatement
beside it -- then the prefetcher and the harness on the device path against the CPU loader path.  Host side:
tests/test_eeg_preprocess_host.py."""
import numpy as np
import pytest
import torch

# the recipe of test_standardise_matches_cpu_normalizer: standard deviations of 5 to 80 uV, offsets of +-2e4 uV
from eeg_filterbank_cases import recordings as _recordings

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


def _taps(F, kind, M, q):
    if kind == "decimate":                                  # scipy.signal.decimate's filter; a half-band low-pass where q = 1
        return F.design_fir(2.0, None, 1.0 / max(q, 2), M)
    if kind == "bandpass":
        return F.design_fir(500.0, 8.0, 30.0, M)
    if kind == "asym":
        return np.array([1.0, 2.0, 0.0, 0.0, 0.0])
    raise KeyError(kind)


def _run(ops, F, x, taps, q, edge, Cout, Tout):
    """-> (device output, mask, float64 oracle, float32 restatement), all (B, Tout, Cout)."""
    dev = _dev()
    h32 = np.asarray(taps, dtype=np.float32)
    out, mask = ops.eeg_preprocess(torch.from_numpy(x).to(dev), torch.from_numpy(h32).to(dev), decimate=q, edge=edge, channels=Cout,
                                   timepoints=Tout)
    ref64, want_mask = F.pad_time(F.preprocess_numpy(x, h32, q, edge, Cout, Tout), Tout)
    ref32, _ = F.pad_time(F.preprocess_numpy(x, h32, q, edge, Cout, Tout, dtype=np.float32), Tout)
    assert out.shape == ref64.shape == (x.shape[0], Tout, Cout) and out.dtype == torch.float32
    assert mask.dtype == torch.bool and mask.shape == (x.shape[0], Tout)
    assert np.array_equal(mask.cpu().numpy(), np.broadcast_to(want_mask, mask.shape))
    return out, mask, ref64, ref32


# (label, B, Cin, Tin, taps, M, q, edge, Cout, Tout)
CASES = [
    ("decimate scipy taps", 2, 33, 130, "decimate", 41, 2, "zero", 33, 65),
    ("decimate channel pad", 2, 33, 131, "decimate", 61, 3, "reflect", 40, 44),
    ("bandpass crops", 2, 70, 300, "bandpass", 101, 1, "reflect", 64, 256),
    ("bandpass crops zero", 2, 70, 300, "bandpass", 101, 1, "zero", 64, 256),
    ("tail pad", 2, 6, 100, "decimate", 21, 4, "reflect", 6, 40),
    ("halo longer than the row", 1, 1, 7, "decimate", 21, 1, "zero", 1, 7),
    ("smallest legal", 1, 1, 4, "decimate", 3, 2, "reflect", 1, 2),
    ("asymmetric taps", 1, 2, 16, "asym", 5, 1, "zero", 2, 16),
    ("one real row length", 2, 122, 1651, "bandpass", 201, 2, "reflect", 122, 826),
]


@pytest.mark.parametrize("label,B,Cin,Tin,kind,M,q,edge,Cout,Tout", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_kernel_matches_the_rule(label, B, Cin, Tin, kind, M, q, edge, Cout, Tout):
    ops, F = _mods()
    from conftest import parity
    x = _recordings(B, Cin, Tin)
    taps = _taps(F, kind, M, q)
    assert len(taps) == M
    out, mask, ref64, ref32 = _run(ops, F, x, taps, q, edge, Cout, Tout)
    parity(f"eeg_preprocess {label}", out, ref32, kind="elem", f64=ref64, ref_is="numpy float32 restatement of the rule")
    Td = -(-Tin // q)
    Tv, Cv = min(Td, Tout), min(Cin, Cout)
    o = out.cpu()
    assert bool((o[:, Tv:] == 0).all()) and bool((o[:, :, Cv:] == 0).all())       # padding and extra channels: exact zeros
    assert bool(torch.isfinite(o).all())
    if Tv > 2:                                              # the statistics are those of the valid part only (the bounds of
        assert float(o[:, :Tv, :Cv].mean(dim=1).abs().max()) < 1e-3               # test_standardise_matches_cpu_normalizer)
        assert float((o[:, :Tv, :Cv].std(dim=1, unbiased=True) - 1).abs().max()) < 1e-3


# (label, B, Cin, Tin, taps, M, q, edge, Cout, Tout): eeg_filterbank_cases' A_one_band, and the row of CASES whose 33 channels cross the
# transpose's 32-channel tile and are padded to 40
DIRECT = [("A_one_band", 2, 5, 64, "bandpass", 21, 1, "reflect", 5, 64), CASES[1]]


@pytest.mark.parametrize("label,B,Cin,Tin,kind,M,q,edge,Cout,Tout", DIRECT, ids=[c[0].replace(" ", "_") for c in DIRECT])
def test_one_band_entry_points_are_the_bank_of_one(label, B, Cin, Tin, kind, M, q, edge, Cout, Tout):
    """No Python caller reaches ign_eeg_preprocess_nct_to_btc / ign_eeg_preprocess_ws_bytes any more (ops.eeg_preprocess goes through
    the bank's entry points), so they are called here directly: the bits of ops.eeg_filterbank(x, h[None]) and the bank's workspace
    size at nb = 1."""
    ops, F = _mods()
    from ign_hip import _lib
    dev = _dev()
    L = _lib.lib()
    x = torch.from_numpy(_recordings(B, Cin, Tin)).to(dev)
    h = torch.from_numpy(_taps(F, kind, M, q).astype(np.float32)).to(dev)
    nbytes = L.ign_eeg_preprocess_ws_bytes(B, Cin, Tin, M, q, Cout, Tout)
    assert nbytes == L.ign_eeg_filterbank_ws_bytes(B, Cin, Tin, M, 1, q, Cout, Tout) == B * min(Cin, Cout) * min(-(-Tin // q), Tout) * 4
    out = torch.full((B, Tout, Cout), float("nan"), device=dev)                    # every element has to be written
    ws = torch.empty(nbytes // 4, device=dev)
    _lib.check(L.ign_eeg_preprocess_nct_to_btc(ops._ptr(x), ops._ptr(h), ops._ptr(out), ops._ptr(ws), B, Cin, Tin, M, q, F.EDGES[edge],
                                               Cout, Tout, 1e-8, ops._stream()), "ign_eeg_preprocess_nct_to_btc")
    want, _ = ops.eeg_filterbank(x, h[None], decimate=q, edge=edge, channels=Cout, timepoints=Tout)
    assert want.shape == out.shape and torch.equal(out, want)
    assert torch.equal(out, ops.eeg_preprocess(x, h, decimate=q, edge=edge, channels=Cout, timepoints=Tout)[0])


def _identity(B=3, C=5, T=50):
    ops, F = _mods()
    dev = _dev()
    x = _recordings(B, C, T)
    xd = torch.from_numpy(x).to(dev)
    ref64 = F.preprocess_numpy(x, np.ones(1), 1, "reflect")
    return ops, xd, torch.ones(1, device=dev), ops.standardise_nct_to_btc(xd), ref64


def test_identity_taps_equal_the_standardise_kernel():
    """taps [1], reflect: the filter does nothing, and the result is ops.standardise_nct_to_btc to 1e-5 per element."""
    ops, xd, one, want, ref64 = _identity()
    out, mask = ops.eeg_preprocess(xd, one)
    assert out.shape == want.shape == (3, 50, 5) and bool(mask.all())
    d64 = lambda t: float(np.abs(t.double().cpu().numpy() - ref64).max())      # noqa: E731
    print(f"identity: |eeg_preprocess - standardise| max {float((out - want).abs().max()):.3e}; against float64: "
          f"eeg_preprocess {d64(out):.3e}, standardise {d64(want):.3e}")
    assert float((out - want).abs().max()) <= 1e-5


@pytest.mark.parametrize("B,C,T", [(3, 5, 50), (2, 33, 301), (2, 122, 1651)])
def test_identity_spec_is_the_default_path_bit_for_bit(B, C, T):
    """A single tap extends nothing, takes no pivot, and the statistics run in the standardise kernel's order (lane-strided sums, the
    butterfly): the same operations in the same order, so taps [1] at the data's own shape give ign_standardise_nct_to_btc's bits --
    in both edge modes, below and above one wave's 64 lanes, with and without explicit channels / timepoints.  Against the float64
    rule that is the standardise kernel's own accuracy: the 5e-4 of test_standardise_matches_cpu_normalizer, same recipe."""
    ops, xd, one, want, ref64 = _identity(B, C, T)
    for kw in (dict(), dict(edge="zero"), dict(channels=C, timepoints=T)):
        out, mask = ops.eeg_preprocess(xd, one, **kw)
        assert torch.equal(out, want) and bool(mask.all()), kw
    assert float(np.abs(out.double().cpu().numpy() - ref64).max()) < 5e-4
    padded, mask = ops.eeg_preprocess(xd, one, channels=C + 3, timepoints=T + 9)       # fitting around it: the same values, zeros
    assert torch.equal(padded[:, :T, :C], want) and bool((padded[:, T:] == 0).all()) and bool((padded[:, :, C:] == 0).all())
    assert bool(mask[:, :T].all()) and not bool(mask[:, T:].any())


def test_asymmetric_taps_keep_their_orientation_on_the_device():
    ops, F = _mods()
    dev = _dev()
    x = np.zeros((1, 1, 16), dtype=np.float32)
    x[0, 0, 7] = 1.0
    h = torch.tensor([1.0, 2.0, 0.0, 0.0, 0.0], device=dev)
    out, _ = ops.eeg_preprocess(torch.from_numpy(x).to(dev), h, edge="zero")
    v = out[0, :, 0].cpu().numpy()
    order = np.argsort(-v)[:2]
    assert sorted(order.tolist()) == [5, 6] and order[0] == 6                       # h[0] lands on n = 5, h[1] = 2 on n = 6
    assert abs((v[6] - v[0]) / (v[5] - v[0]) - 2.0) < 1e-5


def test_two_calls_are_bit_identical_and_strides_do_not_matter():
    ops, F = _mods()
    dev = _dev()
    x = torch.from_numpy(_recordings(3, 37, 301)).to(dev)
    h = torch.from_numpy(F.design_fir(500.0, 8.0, 30.0, 101).astype(np.float32)).to(dev)
    kw = dict(decimate=2, channels=40, timepoints=128)
    a, ma = ops.eeg_preprocess(x, h, **kw)
    b, mb = ops.eeg_preprocess(x, h, **kw)
    assert torch.equal(a, b) and torch.equal(ma, mb)
    wide = torch.zeros(3, 37, 602, device=dev)
    wide[:, :, ::2] = x
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    c, _ = ops.eeg_preprocess(view, h, **kw)
    assert torch.equal(a, c)
    d, _ = ops.eeg_preprocess(x.transpose(0, 1).contiguous().transpose(0, 1), h, **kw)
    assert torch.equal(a, d)
    assert ma.shape == (3, 128) and bool(ma.all())                                 # Td = 151 >= 128: nothing is padding
    e, me = ops.eeg_preprocess(x, h, decimate=2, timepoints=160)
    assert e.shape == (3, 160, 37) and bool(me[:, :151].all()) and not bool(me[:, 151:].any())


def test_ops_refusals_on_the_device():
    ops, F = _mods()
    from ign_hip._lib import IgnError
    dev = _dev()
    x = torch.zeros(1, 2, 10, device=dev)
    with pytest.raises(IgnError, match="odd count"):
        ops.eeg_preprocess(x, torch.ones(4, device=dev))
    with pytest.raises(IgnError, match="reflect extension"):
        ops.eeg_preprocess(x, torch.ones(21, device=dev))
    with pytest.raises(IgnError, match="Tv >= 2"):
        ops.eeg_preprocess(x, torch.ones(1, device=dev), decimate=10)
    with pytest.raises(ValueError):
        ops.eeg_preprocess(x, torch.ones(1, device=dev), edge="wrap")


def test_prefetcher_with_the_preprocess_transform_equals_the_cpu_loader_path(tmp_path):
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
    kw = dict(chain=EEGChain(preprocess="band=8:30,decimate=2,fit", target_channels=8, target_timepoints=120))
    cpu = EEGNpyDataset3Class(str(tmp_path), flag="train", **kw)
    raw = EEGNpyDataset3Class(str(tmp_path), flag="train", raw=True, **kw)
    assert (raw.seq_len, raw.enc_in, raw.pre.Tv) == (120, 8, 100)
    want = list(torch.utils.data.DataLoader(cpu, batch_size=16, shuffle=False, collate_fn=lambda b: collate_fn(b, max_len=cpu.seq_len)))
    loader = torch.utils.data.DataLoader(raw, batch_size=16, shuffle=False, collate_fn=collate_raw, pin_memory=True)
    got = list(DevicePrefetcher(loader, dev, transform=raw.chain.device_transform(dev)))
    assert len(got) == len(want)
    for (a, b, m), (c, d, n) in zip(got, want):
        assert a.is_cuda and a.shape == c.shape == (a.shape[0], 120, 8)
        assert float((a.cpu() - c).abs().max()) < 1e-4
        assert torch.equal(b.cpu(), d) and torch.equal(m.cpu(), n)


def test_harness_trains_on_the_preprocessed_device_pipeline(tmp_path, monkeypatch):
    """Experiment on CHISCO-contract shards with --eeg_preprocess: the device path (raw items, one fused pass in the prefetcher) and
    the CPU item path (numpy in the data set) train to the same losses, on models built for the fitted shape."""
    _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    import run as driver
    from exp.experiment_classification import Experiment
    rng = np.random.RandomState(2)
    y = rng.randint(0, 39, size=96)
    X = (rng.randn(96, 10, 100) * 20 + 300).astype(np.float32)
    X[:, 0, 10:30] += (y // 13)[:, None] * 40.0                 # a class-dependent burst so that the loss moves
    np.save(tmp_path / "X.npy", X)
    np.save(tmp_path / "y.npy", y)
    monkeypatch.chdir(tmp_path)
    losses = {}
    for flag in (True, False):
        args = driver.get_args(["--model", "InterpGN", "--dnn_type", "FCN", "--data", "EEG3", "--data_root", str(tmp_path),
                                "--dataset", "chisco_npy", "--train_epochs", "2", "--batch_size", "32", "--seed", "0", "--amp",
                                "--min_epochs", "5", "--num_workers", "0", "--eeg_preprocess", "decimate=2,fit",
                                "--target_channels", "8", "--target_timepoints", "40"])
        args.device_standardise = flag
        driver.set_seed(0)
        exp = Experiment(args)
        assert args.seq_len == 40 and args.enc_in == 8
        exp.train()
        losses[flag] = exp.validation()
    assert abs(losses[True][0] - losses[False][0]) < 2e-2 and abs(losses[True][1] - losses[False][1]) <= 0.15
