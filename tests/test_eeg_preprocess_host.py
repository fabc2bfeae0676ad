"""Host side of --eeg_preprocess (no device): the ABI of the two entry points, the launcher's refusals with fake pointers, the spec
grammar and its resolution, the FIR designer and the numpy rule against scipy through tests/golden/eeg_preprocess.npz, the
orientation of the convolution, and the CPU loader path.  The GPU side is tests/test_gpu_eeg_preprocess.py."""
import ctypes
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_TOOBIG = -1001, -1003
SYMBOLS = ("ign_eeg_preprocess_ws_bytes", "ign_eeg_preprocess_nct_to_btc")


def _F():
    import speech_imagery_eeg_amd  # noqa: F401
    from utils import eeg_filter
    return eeg_filter


def _lib_or_skip():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    return _lib.lib()


# ---------------------------------------------------------------- ABI
def test_eeg_preprocess_symbols_are_declared_bound_and_exported():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops, _lib
    F = _F()
    text = open(os.path.join(ROOT, "include", "ign_abi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SYMBOLS:
        m = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name        # one ctypes entry per C parameter
    assert _lib.SIGNATURES[SYMBOLS[0]][0] is ctypes.c_size_t
    # the constants the host side restates
    for macro, value in (("IGN_EDGE_REFLECT", ops.EDGE_REFLECT), ("IGN_EDGE_ZERO", ops.EDGE_ZERO), ("IGN_EEG_MAX_TAPS", F.MAX_TAPS),
                         ("IGN_EEG_MAX_DECIMATE", F.MAX_DECIMATE)):
        assert re.search(rf"#define {macro}\s+{value}\b", hdr), macro
    assert F.EDGES == {"reflect": ops.EDGE_REFLECT, "zero": ops.EDGE_ZERO}
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    h = ctypes.CDLL(_lib.lib_path())
    for name in SYMBOLS:
        assert hasattr(h, name), name


def _p(v):
    return ctypes.c_void_p(v)


def _args(**kw):
    a = dict(x=_p(16), taps=_p(32), out=_p(48), ws=_p(64), B=2, Cin=4, Tin=60, M=21, q=2, edge=0, Cout=4, Tout=30, eps=1e-8,
             stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(x=None), E_ARG, b"null pointer"),
    (dict(taps=None), E_ARG, b"null pointer"),
    (dict(out=None), E_ARG, b"null pointer"),
    (dict(ws=None), E_ARG, b"null pointer"),
    (dict(B=0), E_ARG, b"non-positive dimension"),
    (dict(Cin=0), E_ARG, b"non-positive dimension"),
    (dict(Tin=-3), E_ARG, b"non-positive dimension"),
    (dict(Cout=0), E_ARG, b"non-positive dimension"),
    (dict(Tout=0), E_ARG, b"non-positive dimension"),
    (dict(M=20), E_ARG, b"odd count in 1..1023"),
    (dict(M=0), E_ARG, b"odd count in 1..1023"),
    (dict(M=1025, edge=1), E_ARG, b"odd count in 1..1023"),
    (dict(q=0), E_ARG, b"decimation factor q=0 outside 1..16"),
    (dict(q=17), E_ARG, b"decimation factor q=17 outside 1..16"),
    (dict(edge=2), E_ARG, b"neither IGN_EDGE_REFLECT nor IGN_EDGE_ZERO"),
    (dict(M=121), E_ARG, b"reflect extension by R=60"),                    # R = Tin: one more than numpy's 'reflect' takes
    (dict(M=1023, Tin=511), E_ARG, b"reflect extension by R=511"),
    (dict(Tout=1), E_ARG, b"needs Tv >= 2"),
    (dict(Tin=2, M=1, q=2), E_ARG, b"needs Tv >= 2"),                      # Td = 1
    (dict(Tin=20000, M=1023), E_TOOBIG, b"bytes of LDS"),
    (dict(Tin=16000, M=1, q=1, Tout=16000), E_TOOBIG, b"bytes of LDS"),
    (dict(B=65536), E_TOOBIG, b"launch grid"),
])
def test_launcher_refusals_need_no_device(kw, rc, msg):
    h = _lib_or_skip()
    assert h.ign_eeg_preprocess_nct_to_btc(*_args(**kw)) == rc
    assert msg in h.ign_last_error(), h.ign_last_error()


def test_workspace_bytes():
    h = _lib_or_skip()
    # B * min(Cin, Cout) * Tv floats, Tv = min(ceil(Tin / q), Tout)
    assert h.ign_eeg_preprocess_ws_bytes(2, 4, 60, 21, 2, 4, 30) == 2 * 4 * 30 * 4
    assert h.ign_eeg_preprocess_ws_bytes(3, 70, 131, 61, 3, 64, 100) == 3 * 64 * 44 * 4
    assert h.ign_eeg_preprocess_ws_bytes(3, 5, 131, 61, 3, 9, 20) == 3 * 5 * 20 * 4
    assert h.ign_eeg_preprocess_ws_bytes(256, 122, 2000, 413, 2, 122, 1000) == 256 * 122 * 1000 * 4
    for bad in ((0, 4, 60, 21, 2, 4, 30), (2, 4, 60, 20, 2, 4, 30), (2, 4, 60, 21, 0, 4, 30), (2, 4, 60, 21, 17, 4, 30)):
        assert h.ign_eeg_preprocess_ws_bytes(*bad) == 0


def test_ops_refuses_host_tensors_and_bad_edges():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    from ign_hip._lib import IgnError
    with pytest.raises(IgnError, match="no CPU fallback"):
        ops.eeg_preprocess(torch.zeros(1, 2, 8), torch.ones(1))


# ---------------------------------------------------------------- the spec
def test_grammar_and_defaults():
    F = _F()
    S = F.EEGPreprocessSpec
    for text in (None, "", "none", "NONE", " none "):
        s = F.parse_eeg_preprocess(text)
        assert s == S() and not s.active
    assert S() == S(sfreq=500.0, lo=None, hi=None, decimate=1, taps=None, edge="reflect", fit=False)
    assert F.parse_eeg_preprocess("band=8:30,decimate=2,fit") == S(lo=8.0, hi=30.0, decimate=2, fit=True)
    assert F.parse_eeg_preprocess("fit, decimate=2 ,band=8:30") == S(lo=8.0, hi=30.0, decimate=2, fit=True)
    assert F.parse_eeg_preprocess("band=4:") == S(lo=4.0)
    assert F.parse_eeg_preprocess("band=:40") == S(hi=40.0)
    assert F.parse_eeg_preprocess("band=0:40") == S(hi=40.0)                   # a lower edge of 0 Hz is no edge
    assert F.parse_eeg_preprocess("sfreq=250,band=1:40,taps=101,edge=zero") == S(sfreq=250.0, lo=1.0, hi=40.0, taps=101, edge="zero")
    assert F.parse_eeg_preprocess("decimate=4").active and F.parse_eeg_preprocess("fit").active
    assert not F.parse_eeg_preprocess("sfreq=250").active and not F.parse_eeg_preprocess("edge=zero").active
    s = F.parse_eeg_preprocess("decimate=2")
    assert F.parse_eeg_preprocess(s) is s
    assert F.parse_eeg_preprocess("band=:125,decimate=2").hi == 125.0           # exactly the decimated Nyquist rate: allowed


@pytest.mark.parametrize("text", [
    "band=8:130,decimate=2",          # 130 Hz > 500 / (2 * 2): aliases
    "band=8:251",                     # above the Nyquist rate
    "sfreq=200,band=:60,decimate=2",
    "lowpass=40",                     # unknown key
    "fit=1", "decimate", "band=8",    # malformed
    "decimate=2,decimate=3",          # repeated
    "decimate=0", "decimate=17", "decimate=2.5",
    "taps=100,band=8:30", "taps=1025,band=8:30", "taps=21",
    "edge=wrap", "sfreq=0", "band=30:8", "band=x:30", "band=130:,decimate=2",
])
def test_spec_errors(text):
    with pytest.raises(ValueError, match="--eeg_preprocess"):
        _F().parse_eeg_preprocess(text)


def test_default_tap_count_rule(capsys):
    F = _F()
    n = lambda text: F.default_numtaps(F.parse_eeg_preprocess(text))       # noqa: E731
    assert n("decimate=2") == 41 and n("decimate=3") == 61 and n("decimate=16") == 321          # 20 Q + 1: scipy's choice
    assert n("band=8:40,decimate=2") == 207                                 # 3.3 * 500 / 8 = 206.25
    assert n("band=4:40,decimate=2") == 413                                 # 412.5
    assert n("band=:30") == 55                                              # 55.0: already odd
    assert n("band=:33") == 51                                              # 50.0 -> the next odd number
    assert n("sfreq=250,band=10:") == 83                                    # 82.5
    assert n("band=20:,decimate=2") == 83                                   # the lowest non-zero edge, not the implied 125 Hz
    assert n("band=8:30,taps=101") == 101
    assert n("fit") == 1
    assert capsys.readouterr().out == ""
    assert n("band=0.5:40") == 1023                                         # 3301 asked for
    assert "capped at 1023" in capsys.readouterr().out


def test_resolve():
    F = _F()
    r = F.resolve(F.parse_eeg_preprocess("none"), 12, 200)
    assert list(r.taps) == [1.0] and r[1:] == (1, "reflect", 12, 200, 200)
    r = F.resolve("decimate=2,fit", 12, 200, 8, 120)
    assert len(r.taps) == 41 and r[1:] == (2, "reflect", 8, 120, 100)
    r = F.resolve("decimate=3", 12, 200, 8, 120)                            # no fit: the targets stay inert
    assert r[1:] == (3, "reflect", 12, 67, 67)
    r = F.resolve("band=8:30,decimate=2,fit", 122, 1651, 64, 500)
    assert len(r.taps) == 207 and r[1:] == (2, "reflect", 64, 500, 500)
    assert abs(r.taps.sum()) < 2.3e-3 and np.allclose(r.taps, r.taps[::-1])    # symmetric; DC in the Hamming stop band (-53 dB)
    with pytest.raises(ValueError, match="valid time step"):
        F.resolve("decimate=2,fit", 12, 200, 8, 1)                          # Tv = 1
    with pytest.raises(ValueError, match="valid time step"):
        F.resolve("decimate=16,edge=zero", 12, 16)                          # Td = 1
    with pytest.raises(ValueError, match="reflect"):
        F.resolve("band=8:30", 12, 100)                                     # 207 taps reflect 103 samples of 100
    assert len(F.resolve("band=8:30,edge=zero", 12, 100).taps) == 207
    with pytest.raises(ValueError, match="target"):
        F.resolve("fit", 12, 100)


def test_flag_and_data_check():
    import speech_imagery_eeg_amd  # noqa: F401
    import run
    F = _F()
    p = run.build_parser()
    act = {a.option_strings[0]: a for a in p._actions if a.option_strings}["--eeg_preprocess"]
    assert act.default == "none" and act.help
    assert p.parse_args([]).eeg_preprocess == "none"
    assert "--eeg_preprocess" in run.__doc__
    a = run.get_args(["--data", "EEG3", "--eeg_preprocess", "band=8:30,decimate=2,fit"])
    assert F.parse_eeg_preprocess(a.eeg_preprocess).fit
    run.get_args(["--data", "UEA", "--eeg_preprocess", "none"])
    for data in ("UEA", "SYNTH"):
        with pytest.raises(ValueError, match="EEG3"):
            run.get_args(["--data", data, "--eeg_preprocess", "decimate=2"])
    with pytest.raises(ValueError, match="alias"):
        run.get_args(["--data", "EEG", "--eeg_preprocess", "band=8:130,decimate=2"])


# ---------------------------------------------------------------- design and rule against scipy
def _golden():
    from conftest import golden
    return golden("eeg_preprocess")


def test_design_fir_equals_scipy_firwin():
    F, g = _F(), _golden()
    fs = float(g["sfreq"])
    for key, (lo, hi) in (("taps_lowpass_61", (None, 45.0)), ("taps_bandpass_101", (8.0, 30.0)), ("taps_highpass_201", (4.0, None))):
        ref = g[key]
        got = F.design_fir(fs, lo, hi, len(ref))
        assert got.dtype == np.float64 and np.abs(got - ref).max() <= 1e-12, key
    ref = g["taps_decimate_q3"]
    got = F.resolve("decimate=3", 5, 131).taps                              # the default of a decimation-only spec
    assert len(got) == len(ref) == 61 and np.abs(got - ref).max() <= 1e-12
    # the gains firwin scales to: DC, band centre, Nyquist
    k = np.arange(201) - 100
    assert abs(F.design_fir(fs, None, 45.0, 61).sum() - 1) < 1e-12
    assert abs((F.design_fir(fs, 8.0, 30.0, 101) * np.cos(np.pi * (np.arange(101) - 50) * 19.0 / 250)).sum() - 1) < 1e-12
    assert abs((F.design_fir(fs, 4.0, None, 201) * np.cos(np.pi * k)).sum() - 1) < 1e-12
    assert list(F.design_fir(fs, None, 45.0, 1)) == [1.0]
    with pytest.raises(ValueError):
        F.design_fir(fs, None, 45.0, 60)


@pytest.mark.parametrize("q", [2, 3])
def test_rule_with_zero_extension_equals_scipy_decimate(q):
    F, g = _F(), _golden()
    x, ref = g["x"], g[f"decimate_q{q}"]                                    # (2, 5, 131) fp32; (2, 5, ceil(131 / q)) float64
    assert x.dtype == np.float32 and x.shape == (2, 5, 131)
    r = F.resolve(f"decimate={q},edge=zero", 5, 131)
    got = F.preprocess_numpy(x, r.taps, r.q, r.edge, standardise=False)     # (2, Td, 5)
    assert got.shape == (2, -(-131 // q), 5)
    assert np.abs(got.transpose(0, 2, 1) - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.abs(F.filter_decimate(x, r.taps, q, "zero") - ref).max() <= 1e-9 * np.abs(ref).max()


def test_orientation_and_centring():
    """Asymmetric taps on an impulse: a convolution (the taps appear in their own order, not reversed), centred on tap R."""
    F = _F()
    h = np.array([1.0, 2.0, 0.0, 0.0, 0.0])
    x = np.zeros((1, 9))
    x[0, 4] = 1.0
    for edge in ("zero", "reflect"):
        f = F.filter_decimate(x, h, 1, edge)
        assert f.tolist() == [[0, 0, 1, 2, 0, 0, 0, 0, 0]], edge            # f[n] = sum_k h[k] x[n + 2 - k]: h[0] lands on n = 2
    assert F.filter_decimate(x, h, 2, "zero").tolist() == [[0, 1, 0, 0, 0]]   # every second output, starting with n = 0
    assert F.filter_decimate(x, h[::-1].copy(), 1, "zero").tolist() == [[0, 0, 0, 0, 0, 2, 1, 0, 0]]


def test_rule_properties():
    F = _F()
    rng = np.random.RandomState(3)
    x = (rng.randn(2, 6, 100) * 30 + rng.uniform(-2e4, 2e4, size=(2, 6, 1))).astype(np.float32)
    h = F.design_fir(500.0, None, 60.0, 21)
    # reflect extension is numpy's: a constant row passes as sum(h) * constant, so the pivot changes nothing
    ref = np.stack([[np.convolve(np.pad(r, 10, mode="reflect"), h, mode="valid")[::4] for r in s] for s in x.astype(np.float64)])
    f = F.filter_decimate(x, h, 4, "reflect")
    assert f.shape == (2, 6, 25) and np.abs(f - (ref - h.sum() * x[..., :1].astype(np.float64))).max() < 1e-9
    # fit: crop channels, pad channels, crop time; the statistics are those of the kept part
    out = F.preprocess_numpy(x, h, 4, "reflect", channels=8, timepoints=20)
    assert out.shape == (2, 20, 8) and (out[..., 6:] == 0).all()
    assert np.abs(out[..., :6].mean(axis=1)).max() < 1e-12 and np.abs(out[..., :6].std(axis=1, ddof=1) - 1).max() < 1e-8   # eps / std
    z = (f[..., :20] - f[..., :20].mean(-1, keepdims=True)) / (f[..., :20].std(-1, ddof=1, keepdims=True) + 1e-8)
    assert np.abs(out[..., :6] - z.transpose(0, 2, 1)).max() < 1e-12
    assert F.preprocess_numpy(x, h, 4, "reflect", channels=4, timepoints=40).shape == (2, 25, 4)      # Tv = Td: the loader pads
    full, mask = F.pad_time(out, 32)
    assert full.shape == (2, 32, 8) and (full[:, 20:] == 0).all() and mask.tolist() == [True] * 20 + [False] * 12
    # the fp32 restatement with the pivot stays near float64 at 2e4 uV offsets
    o64 = F.preprocess_numpy(x, h.astype(np.float32), 4, "reflect")
    o32 = F.preprocess_numpy(x, h.astype(np.float32), 4, "reflect", dtype=np.float32)
    assert o32.dtype == np.float32 and np.abs(o32 - o64).max() < 2e-5
    # taps [1]: the standardisation alone
    from data_provider.eeg_npy import per_sample_standardise
    ident = F.preprocess_numpy(x, np.ones(1), 1, "reflect")
    assert np.abs(ident - per_sample_standardise(x.astype(np.float64)).transpose(0, 2, 1)).max() < 1e-9
    with pytest.raises(ValueError):
        F.filter_decimate(x, np.ones(4), 1, "zero")
    with pytest.raises(ValueError):
        F.filter_decimate(x, np.ones(201), 1, "reflect")                    # R = 100 = Tin
    assert F.filter_decimate(x, np.ones(201), 1, "zero").shape == (2, 6, 100)


# ---------------------------------------------------------------- the loader
def _shards(tmp_path, n=50, C=12, T=200):
    rng = np.random.RandomState(1)
    X = (rng.randn(n, C, T) * 30 + 500).astype(np.float32)
    np.save(tmp_path / "X.npy", X)
    np.save(tmp_path / "y.npy", rng.randint(0, 39, size=n))
    return X


def _ns(tmp_path, **kw):
    base = dict(task_name="classification", data="EEG3", root_path=str(tmp_path), batch_size=16, num_workers=0, seed=0,
                target_channels=8, target_timepoints=120)
    base.update(kw)
    return Namespace(**base)


def test_none_leaves_the_dataset_and_the_loader_as_they_are(tmp_path):
    import speech_imagery_eeg_amd  # noqa: F401
    from data_provider.data_factory import data_provider
    from data_provider.eeg_chain import EEGChain
    from data_provider.eeg_npy import EEGNpyDataset3Class
    _shards(tmp_path)
    plain = EEGNpyDataset3Class(str(tmp_path), flag="train")
    for raw in (False, True):
        for spec in ("none", None):
            kw = {} if spec is None else dict(eeg_preprocess=spec)
            ds, loader = data_provider(_ns(tmp_path, device_standardise=raw, **kw), "train")
            assert (ds.seq_len, ds.enc_in, ds.num_classes, ds.raw, ds.pre) == (200, 12, 3, raw, None)      # --target_* stay inert
            assert (loader.eeg_chain is ds.chain and loader.eeg_chain.names == []) if raw else loader.eeg_chain is None
            assert ds[0][0].shape == ((12, 200) if raw else (200, 12))
            if not raw:
                assert torch.equal(ds[3][0], plain[3][0])
    ds = EEGNpyDataset3Class(str(tmp_path), flag="train", chain=EEGChain(preprocess="none", target_channels=8, target_timepoints=120))
    assert ds.pre is None and ds.seq_len == 200 and torch.equal(ds[3][0], plain[3][0])


def test_cpu_loader_path_decimates_fits_and_standardises(tmp_path):
    import speech_imagery_eeg_amd  # noqa: F401
    from data_provider.data_factory import data_provider
    F = _F()
    X = _shards(tmp_path)
    for flag in ("train", "val", "test"):                                    # the three loaders are treated alike
        ds, loader = data_provider(_ns(tmp_path, device_standardise=False, eeg_preprocess="decimate=2,fit"), flag)
        assert (ds.seq_len, ds.enc_in) == (120, 8) and ds.pre.Tv == 100 and loader.eeg_chain is None
        x0, y0 = ds[0]
        assert x0.shape == (100, 8) and x0.dtype == torch.float32 and y0.shape == (1,)
    ds, loader = data_provider(_ns(tmp_path, device_standardise=False, eeg_preprocess="decimate=2,fit"), "test")
    got = list(loader)                                                        # the test split is not shuffled
    assert sum(b[0].shape[0] for b in got) == len(ds) == 10
    for xb, yb, mask in got:
        B = xb.shape[0]
        assert xb.shape == (B, 120, 8) and mask.shape == (B, 120) and mask.dtype == torch.bool
        assert bool(mask[:, :100].all()) and not bool(mask[:, 100:].any())
        assert bool((xb[:, 100:] == 0).all())                                 # padding exactly zero
        v = xb[:, :100].double()
        assert float(v.mean(dim=1).abs().max()) < 1e-6 and float((v.std(dim=1, unbiased=True) - 1).abs().max()) < 1e-6
    # the items are the rule applied to the raw rows
    j = ds.idx[0]
    want = F.preprocess_numpy(X[j], ds.pre.taps.astype(np.float32), 2, "reflect", 8, 120)
    assert np.abs(got[0][0][0, :100].numpy() - want).max() < 1e-6
    # a raw data set ships raw items and hands the resolved spec to the loader
    ds, loader = data_provider(_ns(tmp_path, device_standardise=True, eeg_preprocess="decimate=2,fit"), "train")
    assert ds[0][0].shape == (12, 200) and (ds.seq_len, ds.enc_in) == (120, 8)
    assert loader.eeg_chain.names == ["preprocess"] and loader.eeg_chain.stages[0] is ds.pre
    xb, yb, none = next(iter(loader))
    assert xb.shape == (16, 12, 200) and none is None
