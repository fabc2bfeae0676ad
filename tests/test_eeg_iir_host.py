"""Zero-phase IIR stage, host side (no device): the --eeg_iir parser, the scipy-free designer and the float64 rule of
utils/eeg_iir.py against the scipy fixture tests/golden/eeg_iir.npz, the refusals, the ABI of ign_eeg_iir_nct, and the default
``none``, which must leave the loaders, the transforms and fit_alignment exactly as they were."""
import ctypes
import json
import os
import re
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from eeg_iir_cases import CASES, I, case
from eeg_spatial_cases import S, write_shards

G = np.load(os.path.join(ROOT, "tests", "golden", "eeg_iir.npz"))
GRID = np.linspace(0.0, np.pi, 400)
DESIGNS = [(kind, int(n)) for kind in ("low", "high") for n in G["orders"]]


# ------------------------------------------------------------------------------------------------------------------ parser
def test_parser_accepts_every_key_in_any_order():
    m = I()
    for text in (None, "", "none", "None", " none "):
        assert not m.parse_eeg_iir(text).active and m.parse_eeg_iir(text) == m.EEGIIRSpec()
    s = m.parse_eeg_iir("hp=0.5, lp=100 ,order=3,notch=50+100,q=25,sfreq=1000,pad=40")
    assert s == m.EEGIIRSpec(hp=0.5, lp=100.0, order=3, notch=(50.0, 100.0), q=25.0, sfreq=1000.0, pad=40) and s.active
    assert m.parse_eeg_iir("pad=40,sfreq=1000,q=25,notch=50+100,order=3,lp=100,hp=0.5") == s
    assert m.parse_eeg_iir(s) is s and m.parse_eeg_iir(s.text) == s
    d = m.parse_eeg_iir("notch=50")
    assert (d.order, d.q, d.sfreq, d.pad, d.hp, d.lp) == (4, 30.0, 500.0, None, None, None)
    assert m.section_count(m.parse_eeg_iir("hp=1,lp=45,order=8")) == 8 == m.MAX_SECTIONS
    assert m.section_count(m.parse_eeg_iir("hp=1,order=3,notch=50+60")) == 4


@pytest.mark.parametrize("text,msg", [
    ("hq=1", "is not one of"), ("hp", "is not one of"), ("hp=", "is not one of"), ("hp=1,hp=2", "given twice"),
    ("hp=abc", "not a number"), ("order=2.5,hp=1", "not an integer"), ("hp=1,order=0", "outside 1..8"),
    ("hp=1,order=9", "outside 1..8"), ("hp=0", "outside"), ("lp=250", "outside"), ("hp=-1", "outside"),
    ("notch=50+300", "outside"), ("lp=200,sfreq=250", "outside"), ("hp=40,lp=40", "not below"), ("hp=50,lp=40", "not below"),
    ("hp=1,lp=40,order=8,notch=50", "more than 8"), ("notch=10+20+30+40+50+60+70+80+90", "more than 8"),
    ("order=4", "names no filter"), ("notch=50,q=0", "must be positive"), ("hp=1,pad=-1", "negative"),
    ("hp=1,sfreq=0", "sfreq must be positive"), ("hp=nan", "not finite"),
])
def test_parser_refusals(text, msg):
    m = I()
    with pytest.raises(ValueError, match=msg) as e:
        m.parse_eeg_iir(text)
    assert "--eeg_iir" in str(e.value) and "notch=F[+F...]" in str(e.value)           # the grammar is in the text


def test_run_flag_and_its_refusals(tmp_path):
    import speech_imagery_eeg_amd  # noqa: F401
    import run as driver
    base = ["--data_root", str(tmp_path)]
    assert driver.get_args(base + ["--data", "EEG3"]).eeg_iir == "none"
    assert driver.get_args(base + ["--data", "EEG", "--eeg_iir", "hp=1,notch=50"]).eeg_iir == "hp=1,notch=50"
    assert driver.get_args(base + ["--data", "EEG", "--eeg_iir", "hp=1", "--eeg_preprocess", "band=8:30"]).eeg_iir == "hp=1"
    with pytest.raises(ValueError, match="--eeg_iir filters the rows of the raw CHISCO shards"):
        driver.get_args(["--data", "SYNTH", "--eeg_iir", "hp=1"])
    with pytest.raises(ValueError, match="--eeg_preprocess names sfreq=250"):
        driver.get_args(base + ["--data", "EEG", "--eeg_iir", "hp=1", "--eeg_preprocess", "sfreq=250,band=8:30"])
    with pytest.raises(ValueError, match="is not one of"):
        driver.get_args(base + ["--data", "EEG", "--eeg_iir", "highpass=1"])
    assert driver.get_args(["--data", "SYNTH"]).eeg_iir == "none"                    # the default is accepted everywhere
    assert "--eeg_iir" in driver.build_parser().format_help()


# ---------------------------------------------------------------------------------------------------------------- designer
@pytest.mark.parametrize("kind,n", DESIGNS)
def test_butterworth_matches_scipy_and_the_analytic_law(kind, n):
    m = I()
    fc, fs = float(G[f"edge_{kind}"]), float(G["sfreq"])
    sos = m.butter_sos(n, fc, fs, kind)
    assert sos.shape == ((n + 1) // 2, 6) and (sos[:, 3] == 1.0).all()
    if n % 2:
        assert sos[0, 2] == 0.0 and sos[0, 5] == 0.0 and (sos[1:, 5] != 0.0).all()     # the first-order section leads
    m.check_sos(sos)
    h, ref = m.freq_response(sos, GRID), m.freq_response(G[f"sos_{kind}{n}"], GRID)
    d = float(np.abs(h - ref).max())
    print(f"butter {kind} {n}: response distance {d:.2e}")
    assert d <= 1e-10
    assert m.default_pad(sos) == int(G[f"pad_{kind}{n}"])
    w = GRID[1:-1]
    r = (np.tan(w / 2) / np.tan(np.pi * fc / fs)) ** (2 * n)
    law = 1.0 / (1.0 + (r if kind == "low" else 1.0 / r))
    assert np.abs(np.abs(m.freq_response(sos, w)) ** 2 - law).max() <= 1e-10
    # every section has unit gain where the filter passes
    for row in sos:
        assert abs(abs(m.freq_response(row[None], np.asarray([0.0 if kind == "low" else np.pi]))[0]) - 1.0) <= 1e-12


def test_notch_is_iirnotch_and_cascades_are_ordered():
    m = I()
    sos = m.notch_sos(float(G["notch"]), float(G["q"]), float(G["sfreq"]))
    assert np.abs(sos - G["sos_notch"]).max() <= 1e-15 and m.default_pad(sos) == int(G["pad_notch"]) == 9
    w0 = 2 * np.pi * 50.0 / 500.0
    assert abs(m.freq_response(sos, np.asarray([w0]))[0]) <= 1e-12
    assert np.abs(np.abs(m.freq_response(sos, np.asarray([0.0, np.pi]))) - 1.0).max() <= 1e-12
    full = m.design_sos("hp=0.5,lp=40,order=4,notch=50+100,q=20")
    want = np.concatenate([m.butter_sos(4, 0.5, 500.0, "high"), m.butter_sos(4, 40.0, 500.0, "low"), m.notch_sos(50.0, 20.0, 500.0),
                           m.notch_sos(100.0, 20.0, 500.0)])
    assert np.array_equal(full, want) and m.default_pad(full) == 3 * (2 * 6 + 1)
    for spec, pad in (("hp=1,order=1", 6), ("hp=1,order=3", 12), ("hp=0.5,lp=40,order=4,notch=50", 33), ("hp=1,lp=45,order=8", 51),
                      ("hp=0.5,order=4,notch=50", 21), ("lp=100,order=2", 9)):
        assert m.resolve_iir(spec, 1000).pad == pad
    assert {lab: c[4] for lab, c in CASES.items()} == {lab: m.default_pad(m.design_sos(c[3])) for lab, c in CASES.items()}


# -------------------------------------------------------------------------------------------------------------------- rule
@pytest.mark.parametrize("name", [f"{k}{n}" for k, n in DESIGNS] + ["notch"])
def test_rule_with_own_sections_matches_sosfiltfilt(name):
    m = I()
    x = G["x"]
    if name == "notch":
        sos = m.notch_sos(float(G["notch"]), float(G["q"]), float(G["sfreq"]))
    else:
        kind, n = name.rstrip("0123456789"), int(name[-1])
        sos = m.butter_sos(n, float(G[f"edge_{kind}"]), float(G["sfreq"]), kind)
    table, g0 = m.section_table(sos)
    y = m.iir_numpy(x, table, m.default_pad(sos), g0)
    scale = np.abs(x.astype(np.float64) - x[..., :1]).max(axis=-1, keepdims=True)
    d = float((np.abs(y - G[f"y_{name}"]) / scale).max())
    print(f"rule vs sosfiltfilt, {name}: {d:.2e} of max|x - x[0]|")
    assert y.dtype == np.float64 and y.shape == x.shape and d <= 1e-9


def test_constant_rows_map_to_g0_times_the_constant_exactly():
    m = I()
    for spec, g0 in (("hp=0.5", 0.0), ("lp=40", None), ("notch=50", None), ("hp=0.5,lp=40,order=3,notch=50", 0.0)):
        res = m.resolve_iir(spec, 80)
        if g0 is not None:
            assert res.g0 == g0
        else:
            assert abs(res.g0 - 1.0) <= 1e-12
        for c in (0.0, -17.25, 19876.543):
            x = np.full((2, 80), c, dtype=np.float32)
            y = m.iir_numpy(x, res.table, res.pad, res.g0)
            assert np.array_equal(y, res.g0 * x.astype(np.float64))
            assert np.array_equal(res.apply(x), (res.g0 * x.astype(np.float64)).astype(np.float32))


def test_odd_extension_and_single_items():
    m = I()
    u = np.arange(5.0) ** 2
    assert m.odd_extension(u, 0) is u
    assert m.odd_extension(u, 2).tolist() == [-4.0, -1.0, 0.0, 1.0, 4.0, 9.0, 16.0, 32.0 - 9.0, 32.0 - 4.0]
    assert m.odd_extension(u, 4).tolist()[-4:] == [23.0, 28.0, 31.0, 32.0] and m.odd_extension(u, 4).tolist()[:4] == [-16.0, -9.0, -4.0, -1.0]
    k = case("E_odd_order")
    one = m.iir_numpy(k["x"][1, 2], k["table"], k["pad"], k["g0"])                  # a (T,) row alone: the row's own value
    assert np.array_equal(one, k["ref64"][1, 2])


def test_refusals_of_check_sos_and_of_the_resolver():
    m = I()
    ok = m.notch_sos(50.0, 30.0, 500.0)
    assert m.check_sos(ok) is not None
    for bad, msg in ((np.asarray([[1.0, 0, 0, 1.0, -2.0, 1.0]]), "on or outside the unit circle"),          # double pole at z = 1
                     (np.asarray([[1.0, 0, 0, 1.0, 0.0, 1.0]]), "on or outside"),                           # poles at +-i
                     (np.asarray([[1.0, 0, 0, 1.0, -1.0, 0.0]]), "on or outside"),                          # first order, pole at 1
                     (np.asarray([[1.0, 0, 0, 1.0, 0.5, -1.2]]), "on or outside"),
                     (np.asarray([[1.0, 0, 0, 2.0, 0.0, 0.0]]), "a0 = 2"),
                     (np.asarray([[1.0, 0, 0, 1.0, np.nan, 0.0]]), "not finite"),
                     (np.zeros((9, 6)), "expected"), (np.zeros((0, 6)), "expected"), (np.zeros((2, 5)), "expected")):
        with pytest.raises(ValueError, match=msg):
            m.check_sos(bad)
    with pytest.raises(ValueError, match="on or outside"):
        m.resolve_iir("notch=50", 100, sos=np.asarray([[1.0, 0, 0, 1.0, -2.0, 1.0]]))
    assert m.resolve_iir("notch=50", 10).pad == 9
    with pytest.raises(ValueError, match="pad=9 needs rows of more than 9 samples, got 9"):
        m.resolve_iir("notch=50", 9)
    with pytest.raises(ValueError, match="pad=12 needs rows"):
        m.resolve_iir("notch=50,pad=12", 12)
    assert m.resolve_iir("notch=50", 8192 - 18).pad == 9
    with pytest.raises(ValueError, match="exceed the 8192 staged samples"):
        m.resolve_iir("notch=50", 8192 - 17)
    with pytest.raises(ValueError, match="needs rows"):
        m.iir_numpy(np.zeros((2, 5)), ok, 5, 1.0)


def test_section_table_layout_and_the_saved_record(tmp_path):
    m = I()
    res = m.resolve_iir("hp=0.5,lp=40,order=3,notch=50", 300)
    assert res.table.shape == (res.ns, 8) == (5, 8) and res.table.dtype == np.float64 and not res.table[:, 7].any()
    assert np.array_equal(res.table[:, :3], res.sos[:, :3]) and np.array_equal(res.table[:, 3:5], res.sos[:, 4:])
    # zi is the steady state of a unit step: one step from it, with v = G_k, leaves it where it was
    Gk = 1.0
    for b0, b1, b2, a1, a2, z1, z2, _ in res.table:
        y = b0 * Gk + z1
        assert abs((b1 * Gk - a1 * y) + z2 - z1) <= 1e-12 and abs(b2 * Gk - a2 * y - z2) <= 1e-12
        Gk = y
    path = res.save(str(tmp_path))
    rec = json.load(open(path))
    assert os.path.basename(path) == "eeg_iir.json" == m.FILE_NAME
    assert m.parse_eeg_iir(rec["spec"]) == res.spec and rec["pad"] == res.pad == 3 * (2 * 5 + 1 - 2) and rec["g0"] == res.g0
    assert np.array_equal(np.asarray(rec["sos"]), res.sos) and np.array_equal(np.asarray(rec["table"]), res.table)


# --------------------------------------------------------------------------------------------------------------------- ABI
NAMES = ("ign_eeg_iir_lds_bytes", "ign_eeg_iir_nct")
E_ARG, E_TOOBIG = -1001, -1003


def _header_params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    mm = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert mm, f"{name} is not declared in include/ign_abi.h"
    return [p.strip().split()[-1].lstrip("*") for p in mm.group(1).split(",")]


def test_the_symbols_are_in_the_header_in_the_table_and_in_the_docs():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    m = I()
    want = {"ign_eeg_iir_lds_bytes": ["T", "P"],
            "ign_eeg_iir_nct": ["x_nct", "coef", "out_nct", "B", "C", "T", "ns", "P", "g0", "stream"]}
    for name in NAMES:
        assert _header_params(name) == want[name]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(want[name])
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _lib.SIGNATURES["ign_eeg_iir_lds_bytes"][0] is ctypes.c_size_t
    assert _lib.SIGNATURES["ign_eeg_iir_nct"][1][8] is ctypes.c_double                 # g0 travels as a double
    hdr = open(os.path.join(ROOT, "include", "ign_abi.h")).read()
    limits = {k: int(v) for k, v in re.findall(r"#define\s+(IGN_EEG_IIR_MAX_\w+)\s+(\d+)", hdr)}
    assert limits == {"IGN_EEG_IIR_MAX_SECTIONS": m.MAX_SECTIONS, "IGN_EEG_IIR_MAX_ROW": m.MAX_ROW}


def _p(v):
    return ctypes.c_void_p(v)


def _lib_or_skip():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so is not built")
    return _lib.lib()


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(x=None), E_ARG, b"null pointer"), (dict(coef=None), E_ARG, b"null pointer"), (dict(out=None), E_ARG, b"null pointer"),
    (dict(B=0), E_ARG, b"non-positive"), (dict(C=-3), E_ARG, b"non-positive"), (dict(T=0), E_ARG, b"non-positive"),
    (dict(ns=0), E_ARG, b"outside 1..8"), (dict(ns=9), E_ARG, b"outside 1..8"),
    (dict(P=-1), E_ARG, b"P=-1"), (dict(P=60), E_ARG, b"P=60"), (dict(P=61), E_ARG, b"P=61"),
    (dict(T=8175, P=9), E_TOOBIG, b"8193"), (dict(T=5000, P=2000), E_TOOBIG, b"9000"),
    (dict(B=65536, C=65536), E_TOOBIG, b"launch grid"),
])
def test_refusals_return_before_any_launch(kw, rc, msg):
    L = _lib_or_skip()
    a = dict(x=_p(16), coef=_p(32), out=_p(48), B=2, C=4, T=60, ns=2, P=9, g0=1.0, stream=None)
    a.update(kw)
    assert L.ign_eeg_iir_nct(*a.values()) == rc
    assert msg in L.ign_last_error() and b"ign_eeg_iir_nct" in L.ign_last_error()


def test_lds_bytes_is_the_row_as_doubles_plus_the_chunk_transitions():
    L = _lib_or_skip()
    extra = (8 * 6 * 4) * 8                                                        # M^(2^j), j < 6, per section: 2 x 2 doubles each
    assert L.ign_eeg_iir_lds_bytes(1651, 21) == (1651 + 42) * 8 + extra
    assert L.ign_eeg_iir_lds_bytes(8174, 9) == 8192 * 8 + extra and L.ign_eeg_iir_lds_bytes(1, 0) == 8 + extra
    assert L.ign_eeg_iir_lds_bytes(8175, 9) == 0 and L.ign_eeg_iir_lds_bytes(10, 10) == 0 and L.ign_eeg_iir_lds_bytes(10, -1) == 0
    assert L.ign_eeg_iir_lds_bytes(8174, 9) <= 160 * 1024


def test_ops_refuses_cpu_tensors_and_wrong_tables():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ops
    k = case("A_fewer_samples_than_lanes")
    with pytest.raises(_lib.IgnError, match="runs on the MI355X only"):
        ops.eeg_iir(torch.from_numpy(k["x"].copy()), torch.from_numpy(k["table"].copy()), pad=k["pad"], g0=k["g0"])


# -------------------------------------------------------------------------------------------------------- the default `none`
def _ns(tmp_path, **kw):
    base = dict(task_name="classification", data="EEG", root_path=str(tmp_path), batch_size=8, num_workers=0, seed=0,
                target_channels=4, target_timepoints=40)
    base.update(kw)
    return Namespace(**base)


def test_default_builds_the_same_objects_and_never_calls_the_op(tmp_path, monkeypatch):
    import speech_imagery_eeg_amd  # noqa: F401
    from data_provider import device_prefetch
    from data_provider.data_factory import data_provider, ordered_loader
    from data_provider.eeg_npy import collate_raw, per_sample_standardise
    from exp.experiment_classification import Experiment
    from ign_hip import ops

    def boom(*a, **k):
        raise AssertionError("ops.eeg_iir was called under the default")
    monkeypatch.setattr(ops, "eeg_iir", boom)
    monkeypatch.setattr(I(), "design_sos", boom)                                    # nothing is designed either
    X, _, _ = write_shards(str(tmp_path))
    me = SimpleNamespace(device=torch.device("cpu"))
    for kw in ({}, dict(eeg_iir="none"), dict(eeg_iir=None), dict(eeg_iir="")):
        ds, loader = data_provider(_ns(tmp_path, device_standardise=True, **kw), "train")
        assert loader.collate_fn is collate_raw and loader.eeg_chain is ds.chain and loader.eeg_chain.stages == []
        assert ds.iir is None and ordered_loader(loader).eeg_chain is ds.chain
        assert (ds.enc_in, ds.seq_len) == (6, 64) and len(ds[0]) == 2 and next(iter(loader))[2] is None
        pf = Experiment._prefetch(me, loader)
        assert pf.transform is device_prefetch.standardise_raw_batch                # the very function, unwrapped
        ds, loader = data_provider(_ns(tmp_path, device_standardise=False, **kw), "train")
        assert loader.eeg_chain is None and ds.iir is None and Experiment._prefetch(me, loader) is loader
        assert np.array_equal(ds[3][0].numpy(), per_sample_standardise(X[ds.idx[3]]).T)


def test_active_stage_travels_with_the_loader_and_the_cpu_item_path_is_the_rule(tmp_path):
    import speech_imagery_eeg_amd  # noqa: F401
    from data_provider.data_factory import data_provider, ordered_loader
    from data_provider.eeg_npy import collate_raw, per_sample_standardise
    from utils.eeg_filter import filterbank_numpy
    m, s = I(), S()
    X, _, subj = write_shards(str(tmp_path))
    ds, loader = data_provider(_ns(tmp_path, device_standardise=True, eeg_iir="hp=1,notch=50"), "train")
    assert loader.collate_fn is collate_raw and loader.eeg_chain.names == ["iir"] and loader.eeg_chain.stages[0] is ds.iir
    assert ordered_loader(loader).eeg_chain is loader.eeg_chain
    assert ds.iir.pad == 21 and ds.iir.ns == 3 and (ds.enc_in, ds.seq_len) == (6, 64) and len(ds[0]) == 2
    with pytest.raises(ValueError, match="needs rows of more than 64 samples"):
        data_provider(_ns(tmp_path, device_standardise=True, eeg_iir="hp=1,pad=64"), "train")
    with pytest.raises(ValueError, match="--eeg_preprocess names sfreq=250"):
        data_provider(_ns(tmp_path, device_standardise=True, eeg_iir="hp=1", eeg_preprocess="sfreq=250,band=8:30,taps=21"), "train")
    # the CPU item path: spatial (fp32 form), the float64 rule rounded to fp32 once, then what the items were before
    W0 = s.compose("ref=car", 6)
    for pre in (None, "band=8:30,taps=21"):
        kw = {} if pre is None else dict(eeg_preprocess=pre)
        ds, loader = data_provider(_ns(tmp_path, device_standardise=False, eeg_spatial="ref=car", eeg_iir="hp=1,notch=50", **kw), "train")
        assert loader.eeg_chain is None and ds.iir.pad == 21
        for i in (0, 5):
            v = s.spatial_numpy(X[ds.idx[i]], W0[0].astype(np.float32), dtype=np.float32)
            v = m.iir_numpy(v, ds.iir.table, 21, ds.iir.g0).astype(np.float32)
            if pre is None:
                want = per_sample_standardise(v).T
            else:
                p = ds.pre
                want = filterbank_numpy(v, p.taps2d.astype(np.float32), None, p.q, p.edge, p.Cout, p.Tout).astype(np.float32)
            got = ds[i][0]
            assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)


def test_fit_alignment_without_post_is_what_it_was_and_with_post_sees_the_filtered_rows(tmp_path):
    m, s = I(), S()
    X, _, subj = write_shards(str(tmp_path))
    gid = np.searchsorted(np.unique(subj), subj).astype(np.int32)
    batches = [(X[i:i + 8], None, gid[i:i + 8]) for i in range(0, 24, 8)]
    W0 = s.compose("ref=car", 6)
    plain = s.fit_alignment(batches, W0, 3, 1e-6, notice=None)
    assert s.fit_alignment(batches, W0, 3, 1e-6, notice=None, post=None).tobytes() == plain.tobytes()
    assert s.fit_alignment(batches, W0, 3, 1e-6, notice=None, post=lambda y: y).tobytes() == plain.tobytes()
    # today's result, restated: the Gram of W0 . x summed over the batches in float64
    gram, count = np.zeros((3, 6, 6)), np.zeros(3, dtype=np.int64)
    for xb, _, gb in batches:
        gq, cq = s.gram_numpy(s.spatial_numpy(xb, W0), gb, 3)
        gram, count = gram + gq, count + cq
    want = np.stack([s.inverse_root(gram[g] / (float(count[g]) * 64), 1e-6) @ W0[0] for g in range(3)]).astype(np.float32)
    assert want.tobytes() == plain.tobytes()
    res = m.resolve_iir("hp=4,lp=60", 64)
    post = lambda y: m.iir_numpy(y, res.table, res.pad, res.g0)                         # noqa: E731
    W, info = s.fit_alignment(batches, W0, 3, 1e-6, notice=None, post=post, return_info=True)
    assert W.tobytes() != plain.tobytes()
    # the filtered, aligned training trials of every subject have covariance H = I - 11^T / 6 (CAR leaves rank 5)
    H = np.eye(6) - 1.0 / 6
    for g in range(3):
        z = post(s.spatial_numpy(X[gid == g], info["W64"][g]))
        z = z - z.mean(axis=-1, keepdims=True)
        R = np.einsum('bit,bjt->ij', z, z) / (z.shape[0] * 64)
        assert np.abs(R - H).max() <= 1e-6, g
