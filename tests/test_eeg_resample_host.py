"""Rational resampling stage, host side (no device): the --eeg_resample parser, the scipy-free designer and the float64 rule of
utils/eeg_resample.py against the scipy fixture tests/golden/eeg_resample.npz, the phase table, the refusals, the ABI of
ign_eeg_resample_nct, how the stage chains with --eeg_iir and --eeg_preprocess, and the default ``none``, which must leave the data
sets, the loaders and the transforms exactly as they were."""
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
from eeg_resample_cases import CASES, PHASE_LEN, R, case, rows
from eeg_spatial_cases import write_shards

G = np.load(os.path.join(ROOT, "tests", "golden", "eeg_resample.npz"))
FIXTURE = ("a", "b", "c", "e", "f")


# ----------------------------------------------------------------------------------------------------------------- fixture
@pytest.mark.parametrize("name", FIXTURE)
def test_designer_matches_firwin_times_up(name):
    """DESIGN 4.7c's bound for a designer restated without scipy: 1e-12 on taps whose largest is about up / mr <= 1"""
    m = R()
    up, down = int(G[f"up_{name}"]), int(G[f"down_{name}"])
    h = m.design_taps(up, down, int(G["half"]), float(G["beta"]))
    d = float(np.abs(h - G[f"h_{name}"]).max())
    print(f"eeg_resample taps {up}/{down}: {d:.2e} from firwin * up")
    assert h.dtype == np.float64 and h.shape == G[f"h_{name}"].shape == (2 * 10 * max(up, down) + 1,) and d <= 1e-12
    assert abs(h.sum() / up - 1.0) <= 1e-12 and np.array_equal(h, h[::-1])


@pytest.mark.parametrize("name", FIXTURE)
def test_float64_rule_with_unrounded_taps_and_zero_edge_is_resample_poly(name):
    m = R()
    x, up, down = G[f"x_{name}"], int(G[f"up_{name}"]), int(G[f"down_{name}"])
    h = m.design_taps(up, down, int(G["half"]), float(G["beta"]))
    y = m.resample_numpy(x, m.phase_table(h, up), up, down, (len(h) - 1) // 2, "zero")
    x64 = x.astype(np.float64)
    scale = np.abs(x64 - x64[..., :1]).max(axis=-1, keepdims=True)
    d = float((np.abs(y - G[f"y_{name}"]) / scale).max())
    print(f"eeg_resample rule vs resample_poly {up}/{down}: {d:.2e} of max|x - x[0]|")
    assert y.dtype == np.float64 and y.shape == G[f"y_{name}"].shape == x.shape[:-1] + (m.out_length(x.shape[-1], up, down),)
    assert d <= 1e-9


def test_why_the_pivot_the_scratch_numbers_of_the_rule_rederived():
    """Reported, not gated: the per-phase DC gains of 64/125 are unequal, so the offset must not pass through them (the ripple it
    would print, and how far a zero extension of the raw row is off at the edges); the float32 restatement with the pivot is closer
    to float64 than the same chain on the raw row is to its own float64 form."""
    m = R()
    x = rows(1, 3, 1651, seed=3)[0]
    res = m.resolve_resample("rate=256", 1651)
    gains = res.tab.astype(np.float64).sum(axis=1)
    x64 = x.astype(np.float64)
    scale = np.abs(x64 - x64[:, :1]).max(axis=-1, keepdims=True)
    r64 = m.resample_numpy(x, res.tab, 64, 125, res.hl)
    r32 = m.resample_numpy(x, res.tab, 64, 125, res.hl, dtype=np.float32)
    khi, r = np.divmod(np.arange(res.Tout) * 125 + res.hl, 64)

    def raw_chain(mode, dtype):                       # the same chain on the raw row, no pivot
        xe = np.pad(x.astype(dtype), [(0, 0), (res.Lp, res.Lp)], mode=mode)
        acc = np.zeros((3, res.Tout), dtype=dtype)
        for i in range(res.Lp):
            acc += res.tab.astype(dtype)[r, i] * xe[:, khi - i + res.Lp]
        return acc
    raw64, raw32, zero64 = raw_chain("reflect", np.float64), raw_chain("reflect", np.float32), raw_chain("constant", np.float64)
    ripple = float(np.abs(raw64 - r64)[:, res.Lp:-res.Lp].max())
    edges = float(np.abs(zero64 - r64).max())
    e_piv, e_raw = float((np.abs(r32 - r64) / scale).max()), float((np.abs(raw32 - raw64) / scale).max())
    print(f"eeg_resample 64/125: phase DC gains differ from 1 by up to {float(np.abs(gains - 1.0).max()):.2e}; without the pivot the "
          f"offset prints a ripple of up to {ripple:.2f} uV and a zero extension is {edges:.3g} uV off at the edges; fp32 from "
          f"float64 with the pivot {e_piv:.2e} of the centred scale, without {e_raw:.2e}")
    assert np.isfinite([ripple, edges, e_piv, e_raw]).all()


# ------------------------------------------------------------------------------------------------------------------ parser
def test_parser_accepts_every_key_and_takes_the_exact_fraction():
    m = R()
    for text in (None, "", "none", "None", " none "):
        assert not m.parse_eeg_resample(text).active and m.parse_eeg_resample(text) == m.EEGResampleSpec()
    s = m.parse_eeg_resample("rate=256")
    assert s == m.EEGResampleSpec(64, 125, 500.0, 10, 5.0, "reflect") and s.active and s.rate == 256.0
    assert (m.parse_eeg_resample("rate=128").up, m.parse_eeg_resample("rate=128").down) == (32, 125)
    t = m.parse_eeg_resample(" edge=zero, beta=6.5 ,half=4,sfreq=250,rate=256")
    assert t == m.EEGResampleSpec(128, 125, 250.0, 4, 6.5, "zero")
    assert m.parse_eeg_resample("ratio=128/250,sfreq=500") == m.EEGResampleSpec(64, 125)            # lowest terms
    assert m.parse_eeg_resample("rate=0.1,sfreq=0.3").up == 1 and m.parse_eeg_resample("rate=0.1,sfreq=0.3").down == 3   # decimal strings
    assert m.parse_eeg_resample("rate=62.5") == m.EEGResampleSpec(1, 8)
    for spec in (s, t, m.parse_eeg_resample("ratio=3/2")):
        assert m.parse_eeg_resample(spec) is spec and m.parse_eeg_resample(spec.text) == spec
    said = []
    assert m.parse_eeg_resample("rate=500", notice=said.append) == m.EEGResampleSpec() and len(said) == 1 and "no stage" in said[0]
    assert m.parse_eeg_resample("ratio=7/7").text == "none" and not m.parse_eeg_resample("rate=250.0,sfreq=250").active


@pytest.mark.parametrize("text,msg", [
    ("rat=1/2", "is not one of"), ("rate", "is not one of"), ("rate=", "is not one of"), ("rate=256,rate=128", "given twice"),
    ("rate=256,ratio=64/125", "not both"), ("half=4", "not neither"), ("rate=abc", "not a number"), ("rate=1/2", "not a decimal"),
    ("rate=nan", "not a number"), ("rate=0", "rate must be positive"), ("rate=-256", "rate must be positive"),
    ("rate=256,sfreq=0", "sfreq must be positive"), ("rate=256,sfreq=-1", "sfreq must be positive"), ("ratio=64", "is not P/Q"),
    ("ratio=0/3", "must be positive"), ("ratio=2/-3", "must be positive"), ("ratio=2.5/3", "not an integer"),
    ("rate=256,half=0", "outside 1..32"), ("rate=256,half=33", "outside 1..32"), ("rate=256,half=2.5", "not an integer"),
    ("rate=256,beta=0", "beta must be positive"), ("rate=256,beta=-1", "beta must be positive"), ("rate=256,edge=odd", "neither reflect"),
    ("rate=128.5", "more than 8192"), ("ratio=1000/999,half=5", "more than 8192"),
])
def test_parser_refusals_carry_the_grammar(text, msg):
    m = R()
    with pytest.raises(ValueError, match=msg) as e:
        m.parse_eeg_resample(text)
    assert "--eeg_resample" in str(e.value) and "rate=F or ratio=P/Q" in str(e.value)
    if "8192" in msg:
        assert "smaller half=" in str(e.value) and "ratio=P/Q" in str(e.value)


def test_run_flag_and_the_sampling_rates_of_the_three_stages(tmp_path):
    import speech_imagery_eeg_amd  # noqa: F401
    import run as driver
    base = ["--data_root", str(tmp_path), "--data", "EEG"]
    assert driver.get_args(base).eeg_resample == "none" and driver.get_args(["--data", "SYNTH"]).eeg_resample == "none"
    assert driver.get_args(base + ["--eeg_resample", "rate=256"]).eeg_resample == "rate=256"
    assert "--eeg_resample" in driver.build_parser().format_help()
    with pytest.raises(ValueError, match="--eeg_resample resamples the rows of the raw CHISCO shards"):
        driver.get_args(["--data", "SYNTH", "--eeg_resample", "rate=256"])
    with pytest.raises(ValueError, match="is not one of"):
        driver.get_args(base + ["--eeg_resample", "fs=256"])
    # with the stage: --eeg_iir names the input rate, --eeg_preprocess the output rate
    ok = base + ["--eeg_iir", "hp=1,notch=50", "--eeg_resample", "rate=256", "--eeg_preprocess", "band=8:30,sfreq=256"]
    assert driver.get_args(ok).eeg_preprocess == "band=8:30,sfreq=256"
    assert driver.get_args(base + ["--eeg_iir", "hp=1,sfreq=250", "--eeg_resample", "ratio=128/125,sfreq=250", "--eeg_preprocess",
                                   "band=8:30,sfreq=256"]).eeg_iir == "hp=1,sfreq=250"
    with pytest.raises(ValueError, match="leave at 256 Hz, but --eeg_preprocess names sfreq=500"):
        driver.get_args(base + ["--eeg_resample", "rate=256", "--eeg_preprocess", "band=8:30"])
    with pytest.raises(ValueError, match="arrive at sfreq=500 Hz, but --eeg_iir names sfreq=256"):
        driver.get_args(base + ["--eeg_iir", "hp=1,sfreq=256", "--eeg_resample", "rate=256", "--eeg_preprocess", "band=8:30,sfreq=256"])
    # without it (none, or a rate equal to sfreq) the check between the other two is what it was
    for rs in ([], ["--eeg_resample", "none"], ["--eeg_resample", "rate=500"]):
        with pytest.raises(ValueError, match="--eeg_iir: sfreq=500 Hz, but --eeg_preprocess names sfreq=250"):
            driver.get_args(base + rs + ["--eeg_iir", "hp=1", "--eeg_preprocess", "sfreq=250,band=8:30"])
        assert driver.get_args(base + rs + ["--eeg_iir", "hp=1", "--eeg_preprocess", "band=8:30"]).eeg_iir == "hp=1"


# ---------------------------------------------------------------------------------------------------- resolver, table, rule
def test_resolver_lengths_and_table_layout():
    m = R()
    assert {lab: case(lab)["res"].Lp for lab in CASES} == PHASE_LEN
    for Tin, up, down, Tout in ((1651, 64, 125, 846), (50, 2, 3, 34), (50, 3, 2, 75), (97, 1, 2, 49), (100, 128, 125, 103), (125, 64, 125, 64)):
        assert m.out_length(Tin, up, down) == Tout == m.resolve_resample(f"ratio={up}/{down},edge=zero", Tin).Tout
    assert m.resolve_resample("none", 100) is None and m.resolve_resample("rate=500", 100) is None
    for lab in ("A_down_2_3", "B_up_3_2", "D_chisco_row", "E_128_phases", "F_one_phase", "G_half_4"):
        k = case(lab)
        res, up = k["res"], k["up"]
        h32 = res.taps.astype(np.float32)
        M = len(h32)
        assert M == 2 * res.hl + 1 and res.hl == CASES[lab][6] * max(up, k["down"]) and res.Lp == -(-M // up)
        assert res.tab.shape == (up, res.Lp) and res.tab.dtype == np.float32 and res.tab.flags.c_contiguous
        for r in range(up):
            for i in range(res.Lp):
                j = r + i * up
                assert res.tab[r, i] == (h32[j] if j < M else 0.0), (lab, r, i)
        assert m.lds_bytes(res.Tin, up, res.Lp) == 4 * (res.Tin + 2 * res.Lp + up * (res.Lp | 1))
    big = case("I_longest_row")["res"]
    assert m.lds_bytes(big.Tin, 1, big.Lp) == 65536 == m.MAX_LDS_BYTES
    with pytest.raises(ValueError, match="exceed the 64 KB"):
        m.resolve_resample("ratio=1/2", big.Tin + 1)
    assert m.resolve_resample("ratio=2/3", 32).Lp == 31
    with pytest.raises(ValueError, match="reflects 31 samples about each end, but the rows have 31"):
        m.resolve_resample("ratio=2/3", 31)
    assert m.resolve_resample("ratio=2/3,edge=zero", 5).Tout == 4                                    # zeros need no row to mirror
    with pytest.raises(ValueError, match="reflect extension by 31"):
        m.resample_numpy(np.zeros((2, 31)), case("A_down_2_3")["tab"], 2, 3, 30)
    with pytest.raises(ValueError, match="a table of shape"):
        m.resample_numpy(np.zeros((2, 50)), case("A_down_2_3")["tab"], 2, 3, 29)


@pytest.mark.parametrize("label", ["A_down_2_3", "B_up_3_2", "C_64_125_zero", "E_128_phases", "F_one_phase", "G_half_4", "H_shortest_row"])
def test_polyphase_sum_is_the_direct_sum_exactly(label):
    m = R()
    k = case(label)
    h = k["res"].taps.astype(np.float32)
    direct = m.resample_direct(k["x"], h, k["up"], k["down"], k["edge"])
    assert direct.shape == k["ref64"].shape and np.array_equal(direct, k["ref64"])
    one = m.resample_numpy(k["x"][0, -1], k["tab"], k["up"], k["down"], k["hl"], k["edge"])           # a (Tin,) row alone
    assert np.array_equal(one, k["ref64"][0, -1])


def test_constant_rows_give_the_constant_exactly():
    m = R()
    for lab in ("A_down_2_3", "C_64_125_zero", "E_128_phases", "F_one_phase"):
        res = case(lab)["res"]
        for c in (0.0, -17.25, 19876.543):
            x = np.full((2, res.Tin), c, dtype=np.float32)
            assert np.array_equal(m.resample_numpy(x, res.tab, res.up, res.down, res.hl, res.edge), np.full((2, res.Tout), np.float64(x[0, 0])))
            assert np.array_equal(res.apply(x), np.full((2, res.Tout), x[0, 0]))


def test_the_saved_record(tmp_path):
    m = R()
    res = m.resolve_resample("rate=256,half=4", 1651)
    path = res.save(str(tmp_path))
    rec = json.load(open(path))
    assert os.path.basename(path) == "eeg_resample.json" == m.FILE_NAME
    assert m.parse_eeg_resample(rec["spec"]) == res.spec
    assert {k: rec[k] for k in ("sfreq_in", "sfreq_out", "up", "down", "half", "beta", "edge", "Tin", "Tout")} == dict(
        sfreq_in=500.0, sfreq_out=256.0, up=64, down=125, half=4, beta=5.0, edge="reflect", Tin=1651, Tout=846)


# --------------------------------------------------------------------------------------------------------------------- ABI
NAMES = ("ign_eeg_resample_lds_bytes", "ign_eeg_resample_nct")
E_ARG, E_TOOBIG = -1001, -1003


def _header_params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    mm = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert mm, f"{name} is not declared in include/ign_abi.h"
    return [p.strip().split()[-1].lstrip("*") for p in mm.group(1).split(",")]


def test_the_symbols_are_in_the_header_in_the_table_and_in_the_docs():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    m = R()
    want = {"ign_eeg_resample_lds_bytes": ["Tin", "up", "Lp"],
            "ign_eeg_resample_nct": ["x_nct", "tab", "out_nct", "B", "C", "Tin", "Tout", "up", "down", "hl", "Lp", "edge", "stream"]}
    for name in NAMES:
        assert _header_params(name) == want[name]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(want[name])
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _lib.SIGNATURES["ign_eeg_resample_lds_bytes"][0] is ctypes.c_size_t
    hdr = open(os.path.join(ROOT, "include", "ign_abi.h")).read()
    assert int(re.search(r"#define\s+IGN_EEG_RESAMPLE_MAX_TABLE\s+(\d+)", hdr).group(1)) == m.MAX_TABLE == 8192
    assert m.EDGES == {"reflect": int(re.search(r"#define\s+IGN_EDGE_REFLECT\s+(\d+)", hdr).group(1)),
                       "zero": int(re.search(r"#define\s+IGN_EDGE_ZERO\s+(\d+)", hdr).group(1))}


def _p(v):
    return ctypes.c_void_p(v)


def _lib_or_skip():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so is not built")
    return _lib.lib()


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(x=None), E_ARG, b"null pointer"), (dict(tab=None), E_ARG, b"null pointer"), (dict(out=None), E_ARG, b"null pointer"),
    (dict(B=0), E_ARG, b"non-positive"), (dict(C=-3), E_ARG, b"non-positive"), (dict(Tin=0), E_ARG, b"non-positive"),
    (dict(up=0), E_ARG, b"non-positive"), (dict(down=0), E_ARG, b"non-positive"), (dict(hl=-1), E_ARG, b"non-positive"),
    (dict(Lp=0), E_ARG, b"non-positive"),
    (dict(Tout=33), E_ARG, b"ceil(Tin*up/down) = 34"), (dict(Tout=35), E_ARG, b"ceil(Tin*up/down) = 34"),
    (dict(up=4, down=6, Tout=34, Lp=16), E_ARG, b"lowest terms"),
    (dict(Lp=30), E_ARG, b"ceil((2*hl+1)/up) = 31"), (dict(Lp=32), E_ARG, b"ceil((2*hl+1)/up) = 31"),
    (dict(edge=2), E_ARG, b"neither IGN_EDGE_REFLECT"), (dict(edge=-1), E_ARG, b"neither IGN_EDGE_REFLECT"),
    (dict(Tin=31, Tout=21), E_ARG, b"R=31"), (dict(Tin=20, Tout=14), E_ARG, b"R=31"),
    (dict(up=257, down=1000, hl=10000, Lp=78, Tin=1000, Tout=257), E_TOOBIG, b"IGN_EEG_RESAMPLE_MAX_TABLE"),
    (dict(up=1, down=2, hl=20, Lp=41, Tin=16262, Tout=8131), E_TOOBIG, b"bytes of LDS"),
    (dict(up=64, down=125, hl=1250, Lp=40, Tin=13745, Tout=7038), E_TOOBIG, b"bytes of LDS"),
    (dict(B=65536, C=65536), E_TOOBIG, b"launch grid"),
])
def test_refusals_return_before_any_launch(kw, rc, msg):
    L = _lib_or_skip()
    a = dict(x=_p(16), tab=_p(32), out=_p(48), B=2, C=4, Tin=50, Tout=34, up=2, down=3, hl=30, Lp=31, edge=0, stream=None)
    a.update(kw)
    assert L.ign_eeg_resample_nct(*a.values()) == rc
    assert msg in L.ign_last_error() and b"ign_eeg_resample_nct" in L.ign_last_error()


def test_lds_bytes_is_the_extended_row_plus_the_padded_table():
    L, m = _lib_or_skip(), R()
    assert L.ign_eeg_resample_lds_bytes(1651, 64, 40) == 4 * (1651 + 80 + 64 * 41) == m.lds_bytes(1651, 64, 40) == 17420
    assert L.ign_eeg_resample_lds_bytes(50, 3, 21) == 4 * (50 + 42 + 3 * 21)                        # an odd Lp is its own stride
    assert L.ign_eeg_resample_lds_bytes(16261, 1, 41) == 65536 and L.ign_eeg_resample_lds_bytes(16262, 1, 41) == 0
    assert L.ign_eeg_resample_lds_bytes(13680, 64, 40) == 65536 and L.ign_eeg_resample_lds_bytes(13681, 64, 40) == 0
    assert L.ign_eeg_resample_lds_bytes(0, 1, 41) == 0 and L.ign_eeg_resample_lds_bytes(100, 0, 41) == 0
    assert L.ign_eeg_resample_lds_bytes(100, 257, 78) == 0


def test_ops_refuses_cpu_tensors():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ops
    k = case("A_down_2_3")
    with pytest.raises(_lib.IgnError, match="runs on the MI355X only"):
        ops.eeg_resample(torch.from_numpy(k["x"].copy()), torch.from_numpy(k["tab"].copy()), up=2, down=3, half_len=30)


# ------------------------------------------------------------------------------------------------- chaining and the default
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
        raise AssertionError("the resampling stage ran under the default")
    monkeypatch.setattr(ops, "eeg_resample", boom)
    monkeypatch.setattr(R(), "design_taps", boom)                                   # nothing is designed either
    X, _, _ = write_shards(str(tmp_path))
    me = SimpleNamespace(device=torch.device("cpu"))
    for kw in ({}, dict(eeg_resample="none"), dict(eeg_resample=None), dict(eeg_resample=""), dict(eeg_resample="rate=500")):
        ds, loader = data_provider(_ns(tmp_path, device_standardise=True, **kw), "train")
        assert loader.collate_fn is collate_raw and loader.eeg_chain is ds.chain and loader.eeg_chain.stages == []
        assert ds.resample is None and ordered_loader(loader).eeg_chain is ds.chain
        assert (ds.enc_in, ds.seq_len) == (6, 64) and len(ds[0]) == 2 and next(iter(loader))[2] is None
        pf = Experiment._prefetch(me, loader)
        assert pf.transform is device_prefetch.standardise_raw_batch                # the very function, unwrapped
        ds, loader = data_provider(_ns(tmp_path, device_standardise=False, **kw), "train")
        assert loader.eeg_chain is None and ds.resample is None and Experiment._prefetch(me, loader) is loader
        assert np.array_equal(ds[3][0].numpy(), per_sample_standardise(X[ds.idx[3]]).T)
        ds, _ = data_provider(_ns(tmp_path, device_standardise=False, eeg_iir="hp=1", eeg_preprocess="band=8:30,taps=21", **kw), "train")
        assert ds.resample is None and (ds.enc_in, ds.seq_len) == (6, 64)


def test_active_stage_sets_the_shapes_travels_with_the_loader_and_checks_the_rates(tmp_path, capsys):
    import speech_imagery_eeg_amd  # noqa: F401
    from data_provider import device_prefetch
    from data_provider.data_factory import data_provider, ordered_loader
    from data_provider.eeg_npy import collate_raw
    from exp.experiment_classification import Experiment
    write_shards(str(tmp_path))
    ds, loader = data_provider(_ns(tmp_path, device_standardise=True, eeg_resample="rate=256"), "train")
    assert loader.collate_fn is collate_raw and loader.eeg_chain.names == ["resample"] and loader.eeg_chain.stages[0] is ds.resample
    assert ordered_loader(loader).eeg_chain is loader.eeg_chain
    assert (ds.resample.Tin, ds.resample.Tout, ds.resample.Lp) == (64, 33, 40) and (ds.enc_in, ds.seq_len) == (6, 33)
    assert tuple(ds[0][0].shape) == (6, 64)                                         # raw items keep the shards' length
    pf = Experiment._prefetch(SimpleNamespace(device=torch.device("cpu")), loader)
    assert pf.loader is loader and loader.eeg_chain.names == ["resample"]            # the one stage, in front of the standardisation
    assert pf.transform is not device_prefetch.standardise_raw_batch
    # the FIR stage resolves against Tout: without fit its own Td, with fit the target
    ds, loader = data_provider(_ns(tmp_path, device_standardise=True, eeg_iir="hp=1,notch=50", eeg_resample="rate=256",
                                   eeg_preprocess="band=8:30,sfreq=256,taps=21"), "train")
    assert (ds.enc_in, ds.seq_len, ds.pre.Tout, ds.pre.Tv) == (6, 33, 33, 33) and ds.iir.pad == 21
    assert loader.eeg_chain.names == ["iir", "resample", "preprocess"]
    assert all(a is b for a, b in zip(loader.eeg_chain.stages, (ds.iir, ds.resample, ds.pre)))
    ds, _ = data_provider(_ns(tmp_path, device_standardise=True, eeg_resample="rate=256", eeg_preprocess="band=8:30,sfreq=256,taps=21,decimate=2"),
                          "train")
    assert (ds.seq_len, ds.pre.Tout) == (17, 17)
    ds, _ = data_provider(_ns(tmp_path, device_standardise=True, eeg_resample="rate=256", eeg_preprocess="band=8:30,sfreq=256,taps=21,fit"),
                          "train")
    assert (ds.enc_in, ds.seq_len, ds.pre.Tout, ds.pre.Tv) == (4, 40, 40, 33)
    # a FIR filter that fitted the 64-sample row no longer fits the 33-sample one
    with pytest.raises(ValueError, match="taps reflect 40 samples about each end, but the rows have 33"):
        data_provider(_ns(tmp_path, device_standardise=True, eeg_resample="rate=256", eeg_preprocess="band=8:30,sfreq=256,taps=81"), "train")
    with pytest.raises(ValueError, match="leave at 256 Hz, but --eeg_preprocess names sfreq=500"):
        data_provider(_ns(tmp_path, device_standardise=True, eeg_resample="rate=256", eeg_preprocess="band=8:30,taps=21"), "train")
    with pytest.raises(ValueError, match="arrive at sfreq=500 Hz, but --eeg_iir names sfreq=250"):
        data_provider(_ns(tmp_path, device_standardise=True, eeg_resample="rate=256", eeg_iir="hp=1,sfreq=250"), "train")
    with pytest.raises(ValueError, match="--eeg_preprocess names sfreq=250"):       # without the stage: the check that was
        data_provider(_ns(tmp_path, device_standardise=True, eeg_iir="hp=1", eeg_preprocess="sfreq=250,band=8:30,taps=21"), "train")
    with pytest.raises(ValueError, match="reflects 67 samples about each end, but the rows have 64"):
        data_provider(_ns(tmp_path, device_standardise=True, eeg_resample="rate=256,half=17"), "train")
    capsys.readouterr()
    data_provider(_ns(tmp_path, device_standardise=True, eeg_resample="rate=500"), "train")
    assert capsys.readouterr().out.count("no stage") == 1
    data_provider(_ns(tmp_path, device_standardise=True, eeg_resample="rate=500"), "test")
    assert "no stage" not in capsys.readouterr().out


def test_the_cpu_item_is_the_rule(tmp_path):
    import speech_imagery_eeg_amd  # noqa: F401
    from data_provider.data_factory import data_provider
    from data_provider.eeg_npy import per_sample_standardise
    from eeg_iir_cases import I
    from eeg_spatial_cases import S
    from utils.eeg_filter import filterbank_numpy
    m, mi, s = R(), I(), S()
    X, _, _ = write_shards(str(tmp_path))
    W0 = s.compose("ref=car", 6)
    for pre in (None, "band=8:30,sfreq=256,taps=21"):
        kw = {} if pre is None else dict(eeg_preprocess=pre)
        ds, loader = data_provider(_ns(tmp_path, device_standardise=False, eeg_spatial="ref=car", eeg_iir="hp=1,notch=50",
                                       eeg_resample="rate=256", **kw), "train")
        assert loader.eeg_chain is None and ds.seq_len == 33
        rs = ds.resample
        for i in (0, 5):
            v = s.spatial_numpy(X[ds.idx[i]], W0[0].astype(np.float32), dtype=np.float32)
            v = mi.iir_numpy(v, ds.iir.table, 21, ds.iir.g0).astype(np.float32)
            v = m.resample_numpy(v, rs.tab, 64, 125, rs.hl, "reflect").astype(np.float32)
            assert v.shape == (6, 33)
            if pre is None:
                want = per_sample_standardise(v).T
            else:
                p = ds.pre
                want = filterbank_numpy(v, p.taps2d.astype(np.float32), None, p.q, p.edge, p.Cout, p.Tout).astype(np.float32)
            got = ds[i][0]
            assert got.dtype == torch.float32 and tuple(got.shape) == (33, 6) and np.array_equal(got.numpy(), want)
        xb, _, mask = next(iter(loader))
        assert tuple(xb.shape) == (8, 33, 6) and bool(mask.all())
