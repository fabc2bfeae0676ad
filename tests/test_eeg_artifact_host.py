"""Artifact stage, host side (no device): the --eeg_artifact parser, the numpy rule of utils/eeg_artifact.py against a brute-force
restatement written here (sorted() per row, float64 repair), the chain with the stage on (order of calls with recorder ops, one
upload, no gid, the item path to the byte), the record file, the ABI of the three symbols with their refusals, and the default
``none``, which must leave the loaders and the transform exactly as they were."""
import ctypes
import json
import math
import os
import re
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from eeg_artifact_cases import A, CASES, KEYS, RUNS, expected, inputs, plant
from eeg_spatial_cases import write_shards

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ parser
def test_parser_accepts_every_key_in_any_order(tmp_path):
    m = A()
    for text in (None, "", "none", "None", " none "):
        assert not m.parse_eeg_artifact(text).active and m.parse_eeg_artifact(text) == m.EEGArtifactSpec()
    np.save(tmp_path / "w.npy", np.ones((4, 4)))
    path = str(tmp_path / "w.npy")
    s = m.parse_eeg_artifact(f"clip=6, flat=0.01 ,noisy=8,neighbors={path},report")
    assert s == m.EEGArtifactSpec(clip=6.0, flat=0.01, noisy=8.0, neighbors=path, report=True, given=True) and s.active
    assert m.parse_eeg_artifact(f"report,neighbors={path},noisy=8,flat=0.01,clip=6") == s
    assert m.parse_eeg_artifact(s) is s and m.parse_eeg_artifact(s.text) == s
    assert m.parse_eeg_artifact("report").active and m.parse_eeg_artifact("flat=0").flat == 0.0
    d = m.parse_eeg_artifact("clip=4.5")
    assert (d.clip, d.flat, d.noisy, d.neighbors, d.report) == (4.5, None, None, None, False)


def test_parser_refusals(tmp_path):
    m = A()
    np.save(tmp_path / "rect.npy", np.ones((3, 4)))
    np.save(tmp_path / "neg.npy", -np.ones((3, 3)))
    np.save(tmp_path / "nan.npy", np.full((3, 3), np.nan))
    np.save(tmp_path / "cube.npy", np.ones((2, 3, 3)))
    (tmp_path / "text.npy").write_text("not an array")
    for text, msg in [("clap=6", "is not one of"), ("clip", "is not one of"), ("clip=", "is not one of"), ("report=1", "is not one of"),
                      ("clip=6,clip=7", "clip given twice"), ("clip=abc", "clip='abc' is not a number"),
                      ("clip=0", "clip=0 must be positive"), ("clip=-2", "clip=-2 must be positive"), ("clip=inf", "not finite"),
                      ("flat=1", "flat=1 outside [0, 1)"), ("flat=-0.1", "flat=-0.1 outside [0, 1)"),
                      ("noisy=1", "noisy=1 must be above 1"), ("noisy=0.5", "noisy=0.5 must be above 1"),
                      (f"neighbors={tmp_path / 'missing.npy'}", "cannot be read"), (f"neighbors={tmp_path / 'text.npy'}", "cannot be read"),
                      (f"neighbors={tmp_path / 'rect.npy'}", "(3, 4), not a square matrix"),
                      (f"neighbors={tmp_path / 'cube.npy'}", "not a square matrix"),
                      (f"neighbors={tmp_path / 'neg.npy'}", "negative or non-finite"),
                      (f"neighbors={tmp_path / 'nan.npy'}", "negative or non-finite")]:
        with pytest.raises(ValueError) as e:
            m.parse_eeg_artifact(text)
        assert msg in str(e.value) and str(e.value).startswith("--eeg_artifact: "), (text, str(e.value))
    np.save(tmp_path / "w3.npy", np.ones((3, 3)))
    with pytest.raises(ValueError, match="is 3 x 3, the shards have 6 electrodes"):
        m.resolve_artifact(f"neighbors={tmp_path / 'w3.npy'}", 6, 64)
    with pytest.raises(ValueError, match="rows of 16385 samples exceed the 16384"):
        m.resolve_artifact("clip=6", 6, 16385)
    with pytest.raises(ValueError, match="1025 electrodes exceed the 1024"):
        m.resolve_artifact("clip=6", 1025, 64)


def test_run_flag_and_its_refusals(tmp_path):
    import speech_imagery_eeg_amd  # noqa: F401
    import run as driver
    base = ["--data_root", str(tmp_path)]
    assert driver.get_args(base + ["--data", "EEG3"]).eeg_artifact == "none"
    assert driver.get_args(base + ["--data", "EEG", "--eeg_artifact", "clip=6,report"]).eeg_artifact == "clip=6,report"
    with pytest.raises(ValueError) as e:
        driver.get_args(["--data", "SYNTH", "--eeg_artifact", "clip=6"])
    assert str(e.value) == "--eeg_artifact judges the rows of the raw CHISCO shards (--data EEG / EEG3), not --data SYNTH"
    with pytest.raises(ValueError, match="--eeg_preprocess filters the raw CHISCO shards"):                # checked last
        driver.get_args(["--data", "SYNTH", "--eeg_artifact", "clip=6", "--eeg_preprocess", "band=8:30"])
    with pytest.raises(ValueError, match="--eeg_iir: 'hq=1' is not one of"):                               # and parsed last
        driver.get_args(base + ["--data", "EEG", "--eeg_artifact", "clap=6", "--eeg_iir", "hq=1"])
    with pytest.raises(ValueError, match="--eeg_artifact: 'clap=6' is not one of"):
        driver.get_args(base + ["--data", "EEG", "--eeg_artifact", "clap=6"])
    assert driver.get_args(["--data", "SYNTH"]).eeg_artifact == "none"
    assert "--eeg_artifact" in driver.build_parser().format_help()


# -------------------------------------------------------------------------------------------------------------------- rule
def _brute(x, w, clip=None, flat=None, noisy=None):
    """the issue's rule, one sample (C, T), row by row: sorted() in Python, fp32 scalars where the rule is bit for bit, float64 repair"""
    C, T = x.shape
    k = (T - 1) // 2
    m, s, fin = [F32(0)] * C, [F32(0)] * C, [True] * C
    for c in range(C):
        row = [F32(v) for v in x[c]]
        if not all(math.isfinite(v) for v in row):
            fin[c] = False
            continue
        m[c] = sorted(row)[k] + F32(0)
        s[c] = sorted(abs(F32(v - m[c])) for v in row)[k]
    finite = [s[c] for c in range(C) if fin[c]]
    ref = sorted(finite)[(len(finite) - 1) // 2] if finite else F32(0)
    code = []
    for c in range(C):
        if not fin[c]:
            code.append(3)
        elif flat is not None and (s[c] == 0 or s[c] <= F32(F32(flat) * ref)):
            code.append(1)
        elif noisy is not None and s[c] > F32(F32(noisy) * ref):
            code.append(2)
        else:
            code.append(0)
    good = [c for c in range(C) if code[c] == 0]
    if not good:
        code = [4 if v else 0 for v in code]
    y = np.zeros((C, T), dtype=np.float64)
    for c in range(C):
        if not fin[c]:
            continue
        if clip is None:
            y[c] = x[c]
            continue
        r = F32(F32(F32(clip) * F32(1.4826)) * s[c])
        lo, hi = F32(m[c] - r), F32(m[c] + r)
        y[c] = [min(max(F32(v), lo), hi) for v in x[c]]
    for c in range(C):
        if code[c] not in (1, 2, 3):
            continue
        wj = [1.0 if w is None else float(w[c, j]) for j in good]
        if not sum(wj) > 0:
            wj = [1.0] * len(good)
        y[c] = sum(wv * (y[j] - float(m[j])) for wv, j in zip(wj, good)) / sum(wj)
    return y, np.asarray(code, dtype=np.uint8), np.asarray([[m[c], s[c]] for c in range(C)], dtype=np.float32)


SMALL = [(lab, v) for lab, v in RUNS if np.prod(CASES[lab][0]) <= 20000]


@pytest.mark.parametrize("label,variant", SMALL, ids=[f"{a}-{b}" for a, b in SMALL])
def test_rule_is_the_brute_force_restatement(label, variant):
    k = expected(label, variant)
    x, w = inputs(label)
    for b in range(x.shape[0]):
        y, code, stats = _brute(x[b], w, **KEYS[variant])
        assert np.array_equal(k["verdict"][b], code), (b, k["verdict"][b], code)
        assert np.array_equal(k["stats"][b], stats), b
        rep = (code >= 1) & (code <= 3)
        assert np.array_equal(k["y32"][b][~rep].astype(np.float64), y[~rep]) and np.array_equal(k["y64"][b][~rep], y[~rep])
        assert k["y32"].dtype == np.float32 and k["y64"].dtype == np.float64
        if rep.any():
            assert np.abs(k["y64"][b][rep] - y[rep]).max() <= 1e-9 * max(k["scale"][b], 1.0)
            assert (np.abs(k["y32"][b][rep] - y[rep]) <= 2 * k["bound"][b][rep] + 1e-30).all()    # fp32 here: two roundings per term


def test_the_cases_probe_what_they_say():
    v = {lab: expected(lab, vs[0])["verdict"] for lab, (_, vs) in CASES.items()}
    assert v["C_chisco_row"][0, [17, 60, 101]].tolist() == [1, 2, 3] and v["C_chisco_row"][1, [0, 121]].tolist() == [3, 2]
    assert int((v["C_chisco_row"] != 0).sum()) == 5
    assert v["G_nonfinite"][0].tolist() == [3, 3, 3, 3, 0, 0] and v["G_nonfinite"][1].tolist() == [4] * 6
    assert not expected("G_nonfinite", "all")["y32"][1].any()                            # unrepaired and non-finite: zeros
    assert v["H_verdicts_C1"][:, 0].tolist() == [0, 4, 0, 4, 0]
    assert v["H_verdicts_C2"].tolist() == [[0, 0], [4, 4], [4, 4], [4, 4], [0, 2]]       # one flat of two: ref = the LOWER median = 0
    assert v["H_verdicts_C7"][1].tolist() == [1, 0, 0, 0, 0, 0, 2] and set(v["H_verdicts_C7"][2]) == {4}
    assert v["H_verdicts_C7"][3].tolist() == [4] * 7 and v["H_verdicts_C7"][4].tolist() == [0, 0, 0, 2, 0, 0, 0]
    assert v["H_verdicts_C8"][3].tolist() == [4] * 8 and v["H_verdicts_C8"][1].tolist() == [1, 0, 0, 0, 0, 0, 0, 2]
    assert not expected("H_verdicts_C7", "all")["y32"][2, 6].any()
    assert v["I_neighbors"].tolist() == [[0, 0, 2, 0, 0, 1, 3, 0], [3, 0, 0, 0, 0, 0, 0, 0]]
    f = expected("F_ties", "all")
    assert f["verdict"][0].tolist() == [4] * 4 and f["stats"][0, 1].tolist() == [0.0, 0.0] and not np.signbit(f["stats"][0, 1, 0])
    assert expected("F_ties", "clip_only")["verdict"][0].tolist() == [0] * 4 and expected("F_ties", "flat_zero")["verdict"][0].tolist() == [0, 1, 1, 0]
    k = expected("B_64_lower_median", "all")
    assert k["stats"][0, 0, 0] == np.sort(k["x"][0, 0])[31]                              # rank 31 of 64, not the mean of 31 and 32
    c = expected("A_fewer_samples_than_lanes", "all")                                    # the clamp takes the spike down to hi
    assert c["y32"][1, 2, 3] < c["x"][1, 2, 3] - 500 and c["y32"][1, 2, 3] == c["y32"][1, 2].max()
    # the fallback: electrode 5 of case I has no good neighbour of positive weight and is the plain mean of the good rows
    i = expected("I_neighbors", "all")
    good = np.flatnonzero(i["verdict"][0] == 0)
    mean = (i["y64"][0, good] - i["stats"][0, good, 0:1].astype(np.float64)).mean(0)
    assert np.abs(i["y64"][0, 5] - mean).max() <= 1e-9


def test_zero_weights_and_the_diagonal_do_not_enter():
    m = A()
    x, w = inputs("I_neighbors")
    w2 = w.copy()
    np.fill_diagonal(w2, 0.0)
    a, b = m.artifact_numpy(x, w=w, **KEYS["all"]), m.artifact_numpy(x, w=w2, **KEYS["all"])
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    with pytest.raises(ValueError, match="negative or non-finite"):
        m.artifact_numpy(x, w=-w)
    one = m.artifact_numpy(x[0], w=w, **KEYS["all"])                                     # a (C, T) item alone: the sample's own bits
    assert all(np.array_equal(p[0], q) for p, q in zip(a, one))


# ------------------------------------------------------------------------------------------------------------------- chain
class _Recorder:
    """the stage ops and the standardisation, on CPU tensors: what was called, in which order, with what"""

    def __init__(self, monkeypatch):
        from ign_hip import ops
        self.calls = []
        for name in ("eeg_artifact", "eeg_spatial", "eeg_iir", "standardise_nct_to_btc"):
            monkeypatch.setattr(ops, name, getattr(self, name))

    def eeg_artifact(self, x, clip=None, flat=None, noisy=None, neighbors=None):
        self.calls.append(("eeg_artifact", x, neighbors, dict(clip=clip, flat=flat, noisy=noisy)))
        return x + 0.5, torch.zeros(x.shape[:2], dtype=torch.uint8), torch.zeros(*x.shape[:2], 2)

    def eeg_spatial(self, x, W, gid=None):
        self.calls.append(("eeg_spatial", x, W, gid))
        return x + 1.0

    def eeg_iir(self, x, coef, pad, g0):
        self.calls.append(("eeg_iir", x, coef, dict(pad=pad, g0=g0)))
        return x + 2.0

    def standardise_nct_to_btc(self, x):
        self.calls.append(("standardise", x, None, None))
        return x.transpose(1, 2) + 5.0


def _ns(root, raw, **kw):
    return Namespace(task_name="classification", data="EEG", root_path=str(root), batch_size=8, num_workers=0, seed=0,
                     device_standardise=raw, **kw)


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    import speech_imagery_eeg_amd  # noqa: F401
    root = tmp_path_factory.mktemp("artifact")
    X, _, subj = write_shards(str(root), T=100)
    planted = plant(X)
    np.save(root / "X.npy", X)
    w = np.random.RandomState(2).rand(6, 6).astype(np.float32)
    np.save(root / "w.npy", w)
    return Namespace(root=root, X=X, w=w, planted=planted, flag=f"clip=6,flat=0.01,noisy=8,neighbors={root / 'w.npy'}")


def test_the_stage_runs_first_with_one_upload_and_without_gid(shards, monkeypatch):
    from data_provider.data_factory import data_provider
    from data_provider.eeg_chain import ORDER
    from exp.experiment_classification import Experiment
    assert ORDER == ("artifact", "spatial", "iir", "resample", "preprocess")
    rec = _Recorder(monkeypatch)
    ds, loader = data_provider(_ns(shards.root, True, eeg_artifact=shards.flag, eeg_spatial="align=euclid", eeg_iir="hp=1"), "train")
    assert loader.eeg_chain is ds.chain and ds.chain.names == ["artifact", "spatial", "iir"] and ds.chain.stages[0] is ds.artifact
    assert (ds.enc_in, ds.seq_len) == (6, 100)
    ds.spatial.W = np.random.RandomState(1).randn(3, 6, 6).astype(np.float32)
    pf = Experiment._prefetch(Namespace(device=torch.device("cpu")), loader)
    torch.manual_seed(2)
    raw = list(loader)
    torch.manual_seed(2)
    got = list(pf)
    assert len(got) == len(raw) == 3
    same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))      # noqa: E731  (one trial holds a NaN)
    assert [c[0] for c in rec.calls] == ["eeg_artifact", "eeg_spatial", "eeg_iir", "standardise"] * 3
    for b, (x, y, gid) in enumerate(raw):
        art, sp, iir, last = rec.calls[4 * b:4 * b + 4]
        assert same(art[1], x) and art[1].dtype == torch.float32 and art[3] == dict(clip=6.0, flat=0.01, noisy=8.0)
        assert torch.equal(art[2], torch.from_numpy(shards.w)) and art[2].dtype == torch.float32
        assert not any(torch.is_tensor(v) and v.dtype == torch.int32 for v in (art[1], art[2], *art[3].values()))   # no group ids
        assert same(sp[1], x + 0.5) and torch.equal(sp[3], gid) and gid.dtype == torch.int32
        assert same(iir[1], x + 1.5) and same(last[1], x + 3.5)
        assert same(got[b][0], (x + 8.5).transpose(1, 2)) and torch.equal(got[b][1], y)
    assert len({id(rec.calls[4 * b][2]) for b in range(3)}) == 1                         # one table object over the three batches


def test_item_path_is_the_rules_composed_by_hand(shards):
    from data_provider.data_factory import data_provider
    from data_provider.eeg_npy import per_sample_standardise
    from utils.eeg_iir import iir_numpy
    from utils.eeg_spatial import compose, spatial_numpy
    m = A()
    ds, loader = data_provider(_ns(shards.root, False, eeg_artifact=shards.flag, eeg_spatial="ref=car", eeg_iir="hp=1"), "train")
    assert loader.eeg_chain is None and ds.chain.names == ["artifact", "spatial", "iir"]
    W0 = compose("ref=car", 6)
    seen = set()
    for i in range(len(ds)):
        j = ds.idx[i]
        v, verdict, _ = m.artifact_numpy(shards.X[j], w=shards.w, clip=6.0, flat=0.01, noisy=8.0)
        seen |= set(verdict.tolist())
        v = spatial_numpy(v, W0[0].astype(np.float32), dtype=np.float32)
        v = iir_numpy(v, ds.iir.table, ds.iir.pad, ds.iir.g0).astype(np.float32)
        want = per_sample_standardise(v).T
        got = ds[i][0].numpy()
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes() and np.isfinite(got).all()
    assert seen >= {0, 1, 2}
    plain, _ = data_provider(_ns(shards.root, False, eeg_spatial="ref=car", eeg_iir="hp=1"), "train")
    k = list(plain.idx).index(shards.planted["nan"][0]) if shards.planted["nan"][0] in plain.idx else None
    if k is not None:
        assert not np.isfinite(plain[k][0].numpy()).all()                                # what the stage is for


def test_save_writes_exactly_one_more_record_and_the_report(shards, tmp_path):
    from data_provider.eeg_chain import EEGChain
    m = A()
    root = str(shards.root)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    before = EEGChain(spatial="ref=car", iir="hp=1").resolve(6, 100, root, 24).save(str(tmp_path / "a"))
    chain = EEGChain(spatial="ref=car", iir="hp=1", artifact=shards.flag + ",report").resolve(6, 100, root, 24)
    stage = chain.stage("artifact")
    rep = stage.report_pass([(shards.X[i:i + 8], None, None) for i in range(0, 24, 8)])
    after = chain.save(str(tmp_path / "b"))
    assert sorted(os.listdir(tmp_path / "b")) == sorted(os.listdir(tmp_path / "a") + ["eeg_artifact.json"])
    assert [os.path.basename(p) for p in after] == ["eeg_artifact.json"] + [os.path.basename(p) for p in before]
    rec = json.load(open(tmp_path / "b" / "eeg_artifact.json"))
    assert m.parse_eeg_artifact(rec["spec"]) == stage.spec and rec["weights"]["shape"] == [6, 6] and len(rec["weights"]["sha256"]) == 64
    assert rec["report"] == rep and rep["trials"] == 24 and rep["repaired_trials"] == 24
    assert rep["flat"] == [0, 24, 0, 0, 0, 0] and rep["nonfinite"] == [0, 0, 1, 0, 0, 0] and rep["unrepaired"] == [0] * 6
    assert rep["noisy"] == [0, 0, 0, 0, len(shards.planted["noisy_trials"]), 0]
    lines = stage.report_lines()
    assert "24 training trials, 24 (100.0%) with a repaired electrode" in lines[0] and len(lines) == 2 + 3
    assert lines[2].split()[1:] == ["1", "24", "0", "0", "0"]                            # the railed electrode leads the table
    plain = EEGChain(artifact="clip=6").resolve(6, 100, root, 24)
    (tmp_path / "c").mkdir()
    plain.save(str(tmp_path / "c"))
    rec = json.load(open(tmp_path / "c" / "eeg_artifact.json"))
    assert rec["weights"] is None and "report" not in rec and rec["clip"] == 6.0


def test_alignment_is_fitted_on_the_repaired_rows(shards, monkeypatch):
    import speech_imagery_eeg_amd  # noqa: F401
    from exp.experiment_classification import Experiment
    from utils import eeg_spatial
    seen = []
    real = eeg_spatial.fit_alignment

    def spy(batches, *a, **k):
        batches = list(batches)
        seen.append(batches)
        return real(batches, *a, **k)
    monkeypatch.setattr(eeg_spatial, "fit_alignment", spy)
    m = A()
    me = SimpleNamespace(args=_ns(shards.root, False, eeg_artifact=shards.flag, eeg_spatial="align=euclid"), device=torch.device("cpu"),
                         rank=1)
    me._fit_eeg_spatial = lambda: Experiment._fit_eeg_spatial(me)
    Experiment._load_data(me)
    assert me.train_data.spatial.fitted and np.isfinite(me.train_data.spatial.W).all()
    (fixed,) = seen
    X = shards.X[me.train_data.idx[:8]]
    assert not np.isfinite(shards.X[me.train_data.idx]).all()                            # the raw training trials hold the NaN
    assert np.array_equal(np.asarray(fixed[0][0]), m.artifact_numpy(X, w=shards.w, clip=6.0, flat=0.01, noisy=8.0)[0])
    assert all(np.isfinite(np.asarray(b[0])).all() for b in fixed)


# --------------------------------------------------------------------------------------------------------------------- ABI
NAMES = ("ign_eeg_artifact_lds_bytes", "ign_eeg_artifact_stats_nct", "ign_eeg_artifact_apply_nct")
E_ARG, E_TOOBIG = -1001, -1003


def _header_params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    mm = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert mm, f"{name} is not declared in include/ign_abi.h"
    return [p.strip().split()[-1].lstrip("*") for p in mm.group(1).split(",")]


def test_the_symbols_are_in_the_header_in_the_table_and_in_the_docs():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    m = A()
    want = {"ign_eeg_artifact_lds_bytes": ["T"],
            "ign_eeg_artifact_stats_nct": ["x_nct", "stats", "flags", "B", "C", "T", "stream"],
            "ign_eeg_artifact_apply_nct": ["x_nct", "stats", "flags", "w", "out_nct", "verdict", "B", "C", "T", "clip", "flat", "noisy",
                                           "stream"]}
    for name in NAMES:
        assert _header_params(name) == want[name]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(want[name])
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _lib.SIGNATURES["ign_eeg_artifact_lds_bytes"][0] is ctypes.c_size_t
    assert _lib.SIGNATURES["ign_eeg_artifact_apply_nct"][1][9:12] == [ctypes.c_float] * 3
    hdr = open(os.path.join(ROOT, "include", "ign_abi.h")).read()
    limits = {k: int(v) for k, v in re.findall(r"#define\s+(IGN_EEG_ARTIFACT_MAX_\w+)\s+(\d+)", hdr)}
    assert limits == {"IGN_EEG_ARTIFACT_MAX_ROW": m.MAX_ROW, "IGN_EEG_ARTIFACT_MAX_CHANNELS": m.MAX_CHANNELS}


def _p(v):
    return ctypes.c_void_p(v)


def _lib_or_skip():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so is not built")
    return _lib.lib()


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(x=None), E_ARG, b"null pointer"), (dict(stats=None), E_ARG, b"null pointer"), (dict(flags=None), E_ARG, b"null pointer"),
    (dict(B=0), E_ARG, b"non-positive"), (dict(C=-3), E_ARG, b"non-positive"), (dict(T=0), E_ARG, b"non-positive"),
    (dict(T=16385), E_TOOBIG, b"T=16385"), (dict(C=1025), E_TOOBIG, b"C=1025"), (dict(B=1 << 22, C=1024), E_TOOBIG, b"launch grid"),
])
def test_stats_refusals_return_before_any_launch(kw, rc, msg):
    L = _lib_or_skip()
    a = dict(x=_p(16), stats=_p(32), flags=_p(48), B=2, C=4, T=60, stream=None)
    a.update(kw)
    assert L.ign_eeg_artifact_stats_nct(*a.values()) == rc
    assert msg in L.ign_last_error() and b"ign_eeg_artifact_stats_nct" in L.ign_last_error()


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(x=None), E_ARG, b"null pointer"), (dict(stats=None), E_ARG, b"null pointer"), (dict(flags=None), E_ARG, b"null pointer"),
    (dict(out=None), E_ARG, b"null pointer"), (dict(verdict=None), E_ARG, b"null pointer"),
    (dict(B=0), E_ARG, b"non-positive"), (dict(C=0), E_ARG, b"non-positive"), (dict(T=-1), E_ARG, b"non-positive"),
    (dict(T=16385), E_TOOBIG, b"T=16385"), (dict(C=1025), E_TOOBIG, b"C=1025"), (dict(B=1 << 22, C=1024), E_TOOBIG, b"launch grid"),
    (dict(B=1 << 24, C=1, T=16384), E_TOOBIG, b"launch grid"),
])
def test_apply_refusals_return_before_any_launch(kw, rc, msg):
    L = _lib_or_skip()
    a = dict(x=_p(16), stats=_p(32), flags=_p(48), w=None, out=_p(64), verdict=_p(80), B=2, C=4, T=60, clip=6.0, flat=0.01, noisy=8.0,
             stream=None)
    a.update(kw)
    assert L.ign_eeg_artifact_apply_nct(*a.values()) == rc
    assert msg in L.ign_last_error() and b"ign_eeg_artifact_apply_nct" in L.ign_last_error()


def test_lds_bytes_is_the_row_of_keys_plus_the_waves_counts():
    L = _lib_or_skip()
    extra = 2 * 4 * 4                                                                 # two slots of four wave counts
    assert L.ign_eeg_artifact_lds_bytes(1) == 4 + extra and L.ign_eeg_artifact_lds_bytes(1651) == 1651 * 4 + extra
    assert L.ign_eeg_artifact_lds_bytes(16384) == 65536 + extra <= 160 * 1024
    assert L.ign_eeg_artifact_lds_bytes(16385) == 0 and L.ign_eeg_artifact_lds_bytes(0) == 0 and L.ign_eeg_artifact_lds_bytes(-4) == 0


def test_ops_refuses_cpu_tensors():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ops
    x, _ = inputs("A_fewer_samples_than_lanes")
    with pytest.raises(_lib.IgnError, match="runs on the MI355X only"):
        ops.eeg_artifact(torch.from_numpy(x.copy()), clip=6.0)
    with pytest.raises(_lib.IgnError, match="runs on the MI355X only"):
        A().resolve_artifact("clip=6", 3, 5).device_fn("cpu")(torch.from_numpy(x.copy()), None)


# -------------------------------------------------------------------------------------------------------- the default `none`
def test_default_builds_the_same_objects_and_never_calls_the_op(tmp_path, monkeypatch):
    import speech_imagery_eeg_amd  # noqa: F401
    from data_provider import device_prefetch
    from data_provider.data_factory import data_provider, ordered_loader
    from data_provider.eeg_npy import collate_raw, per_sample_standardise
    from exp.experiment_classification import Experiment
    from ign_hip import ops

    def boom(*a, **k):
        raise AssertionError("the artifact stage ran under the default")
    monkeypatch.setattr(ops, "eeg_artifact", boom)
    from data_provider import eeg_chain
    monkeypatch.setattr(A(), "load_neighbors", boom)                                  # no file is read
    monkeypatch.setattr(eeg_chain, "resolve_artifact", boom)                          # no table is built
    monkeypatch.setattr(A(), "artifact_numpy", boom)
    X, _, _ = write_shards(str(tmp_path))
    me = SimpleNamespace(device=torch.device("cpu"), rank=0)
    for kw in ({}, dict(eeg_artifact="none"), dict(eeg_artifact=None), dict(eeg_artifact="")):
        ds, loader = data_provider(_ns(tmp_path, True, **kw), "train")
        assert loader.collate_fn is collate_raw and loader.eeg_chain is ds.chain and loader.eeg_chain.stages == []
        assert ds.artifact is None and ordered_loader(loader).eeg_chain is ds.chain and ds.chain.names == []
        assert (ds.enc_in, ds.seq_len) == (6, 64) and len(ds[0]) == 2 and next(iter(loader))[2] is None
        assert Experiment._prefetch(me, loader).transform is device_prefetch.standardise_raw_batch        # the very function, unwrapped
        assert ds.chain.save(str(tmp_path)) == []
        me.train_data = ds
        assert Experiment._report_eeg_artifact(me) is None
        ds, loader = data_provider(_ns(tmp_path, False, **kw), "train")
        assert loader.eeg_chain is None and ds.artifact is None and Experiment._prefetch(me, loader) is loader
        assert np.array_equal(ds[3][0].numpy(), per_sample_standardise(X[ds.idx[3]]).T)
    assert sorted(os.listdir(tmp_path)) == ["X.npy", "subject.npy", "y.npy"]
