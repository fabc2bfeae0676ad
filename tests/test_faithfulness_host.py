"""Faithfulness curves on the host (no GPU): the numpy rule of utils/faithfulness.py (exact counts, nested sets, ties to the lowest
index, the k = 0 sentinel, empty samples) and its lexsort restatement; the --faithfulness parser; the ABI of the two entry points and
their refusals, which return before any launch; the wiring of faithfulness_curves / Experiment.faithfulness / run.py against
recording stand-ins; and that the case table reaches every path of the select kernel's launch geometry.  The GPU side is
tests/test_gpu_faithfulness.py; the cases are tests/faithfulness_cases.py."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, make_cfg
from faithfulness_cases import (KEY_PASSES, KINDS, MAX_K, SIZES, THREADS, TRIP, UNROLL, build, index_passes, lexsort_rule, passes,
                                rank_cases, same_bits, trips)

import speech_imagery_eeg_amd  # noqa: F401
from utils import faithfulness as F

RANK, PERTURB = "ign_rank_threshold", "ign_perturb_btc"
E_ARG, E_TOOBIG = -1001, -1003
SMALL = [c for c in rank_cases() if c["T"] * c["Cs"] <= TRIP + 2]


def _lib_or_skip():
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "ign_abi.h")).read()


def _header_params(name):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
    assert m, name
    return [re.split(r"[\s*]+", p.strip())[-1] for p in m.group(1).split(",")]


# ---------------------------------------------------------------- the rule
def test_key_is_a_total_order_on_bit_patterns():
    v = np.array([-np.nan, -np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf, np.nan], np.float32)
    v[0] = np.frombuffer(np.uint32(0xffc00000).tobytes(), np.float32)[0]
    v[-1] = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]
    key = F.key_of(v)
    assert key.dtype == np.uint32 and (np.diff(key.astype(np.int64)) > 0).all()          # strictly ascending, -0 below +0
    assert key[4] == 0x7fffffff and key[5] == 0x80000000


@pytest.mark.parametrize("case", SMALL, ids=lambda c: f"{c['T']}x{c['Cs']}-{c['kind']}-nk{c['nk']}-B{c['B']}{'-ragged' if c['ragged'] else ''}")
def test_rule_counts_nesting_ties_and_lexsort(case):
    S, k, lengths, n_b = build(case)
    B, T, Cs = S.shape
    thr_key, thr_idx = F.rank_rule(S, k, lengths)
    assert thr_key.dtype == np.uint32 and thr_idx.dtype == np.int32 and thr_key.shape == thr_idx.shape == k.shape
    ref_key, ref_idx = lexsort_rule(S, k, lengths)
    assert np.array_equal(thr_key, ref_key) and np.array_equal(thr_idx, ref_idx)
    keys = F.key_of(S.reshape(B, -1))
    sets = [F.selected_rule(S, thr_key, thr_idx, j, lengths) for j in range(case["nk"])]
    for b in range(B):
        kc = np.clip(k[b].astype(np.int64), 0, n_b[b])
        for j in range(case["nk"]):
            sel = sets[j][b]
            assert sel.sum() == kc[j] == min(max(int(k[b, j]), 0), n_b[b])              # the exact count
            assert not sel[n_b[b]:].any()
            if kc[j] == 0:
                assert thr_key[b, j] == 0xffffffff and thr_idx[b, j] == -1             # the sentinel
                continue
            cut = keys[b][sel].min()
            assert (keys[b][:n_b[b]][~sel[:n_b[b]]] <= cut).all()                     # nothing left out outranks the set
            tied = np.flatnonzero((keys[b] == cut)[:n_b[b]])
            took = np.flatnonzero(sel & (keys[b] == cut))
            assert np.array_equal(took, tied[:len(took)])                              # ties go to the lowest indices
            assert thr_idx[b, j] == took[-1] and thr_key[b, j] == cut
        order = np.argsort(kc, kind="stable")                                          # ascending k: nested sets
        for lo, hi in zip(order[:-1], order[1:]):
            assert not (sets[lo][b] & ~sets[hi][b]).any()
            if kc[lo] == kc[hi]:
                assert np.array_equal(sets[lo][b], sets[hi][b])                        # duplicate k: the same set


def test_rule_handles_empty_samples_and_all_equal_rows():
    S = np.full((3, 5, 2), 0.5, np.float32)
    k = np.array([[0, 3, 10, 99]] * 3, np.int32)
    key, idx = F.rank_rule(S, k, lengths=np.array([5, 0, 2], np.int32))
    half = F.key_of(np.float32(0.5).reshape(1))[0]
    assert idx.tolist() == [[-1, 2, 9, 9], [-1, -1, -1, -1], [-1, 2, 3, 3]]
    assert key.tolist() == [[0xffffffff, half, half, half], [0xffffffff] * 4, [0xffffffff, half, half, half]]
    for j, want in enumerate([[0, 0, 0], [3, 0, 3], [10, 0, 4], [10, 0, 4]]):
        assert F.selected_rule(S, key, idx, j, np.array([5, 0, 2])).sum(1).tolist() == want


@pytest.mark.parametrize("Cs", [1, 3])
def test_perturb_rule_properties(Cs):
    rng = np.random.default_rng(Cs)
    B, T, C = 4, 9, 3
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    x[0, 0, 0] = np.nan
    x[2, 8, 1] = np.frombuffer(np.uint32(0x7fc00123).tobytes(), np.float32)[0]
    S = rng.integers(0, 3, (B, T, Cs)).astype(np.float32)
    lengths = np.array([9, 0, 4, 12], np.int32)
    n_b = np.clip(lengths, 0, T).astype(np.int64) * Cs
    k = np.stack([np.array([0, 1, n // 2, n, n + 1]) for n in n_b]).astype(np.int32)
    key, idx = F.rank_rule(S, k, lengths)
    fill = rng.standard_normal((B, C)).astype(np.float32)
    xb = x.view(np.uint32)
    for j in range(k.shape[1]):
        dele = F.perturb_rule(x, S, key, idx, j, fill=fill, lengths=lengths)
        ins = F.perturb_rule(x, S, key, idx, j, fill=fill, insert=True, lengths=lengths)
        dz, iz = dele.view(np.uint32), ins.view(np.uint32)
        fb = np.broadcast_to(fill.view(np.uint32)[:, None, :], x.shape)
        inside = np.arange(T)[None, :, None] < np.clip(lengths, 0, T)[:, None, None]
        inside = np.broadcast_to(inside, x.shape)
        assert np.array_equal(dz[~inside], xb[~inside]) and np.array_equal(iz[~inside], xb[~inside])      # padding copied through
        put_d, put_i = (dz == fb) & (dz != xb), (iz == fb) & (iz != xb)
        assert not (put_d & put_i).any() and ((dz == xb) | (dz == fb)).all() and ((iz == xb) | (iz == fb)).all()
        assert np.array_equal(np.where(inside, np.where(dz == xb, iz, dz), xb)[inside], fb[inside])      # complements
        kc = np.minimum(np.maximum(k[:, j], 0), n_b)
        assert ((dz != xb).sum((1, 2)) == kc * (C // Cs)).all()                                          # the exact number of cells
        assert same_bits(F.perturb_rule(x, S, key, idx, j, lengths=lengths),
                         F.perturb_rule(x, S, key, idx, j, fill=np.zeros((B, C), np.float32), lengths=lengths))
    assert same_bits(F.perturb_rule(x, S, key, idx, 0, fill=fill, lengths=lengths), x)                   # k = 0 deletes nothing


# ---------------------------------------------------------------- the case table against the launch geometry
def test_case_table_reaches_every_path_of_the_select_kernel():
    src = open(os.path.join(ROOT, "speech-imagery-eeg_amd", "csrc", "ign_faithfulness.hip")).read()
    assert re.search(r"RT_THREADS\s*=\s*(\d+)", src).group(1) == str(THREADS)
    assert re.search(r"RT_UNROLL\s*=\s*(\d+)", src).group(1) == str(UNROLL)
    assert "npass = 4 + ibits / 8" in src and KEY_PASSES == 4 and TRIP == THREADS * UNROLL
    ns = sorted({T * Cs for T, Cs in SIZES})
    assert 1 in ns and TRIP - 1 in ns and TRIP in ns and TRIP + 1 in ns                # one element; below, at, above one trip
    assert max(trips(n) for n in ns) >= 3 and {trips(n) for n in ns} >= {1, 2, 3}        # several trips
    assert {index_passes(n) for n in ns} == {0, 1, 2, 3}                                 # every count of index passes
    assert index_passes(256) == 1 and index_passes(257) == 2 and index_passes(65536) == 2 and index_passes(65537) == 3
    assert passes(1) == 4 and passes(TRIP) == 6
    cases = rank_cases()
    assert {c["kind"] for c in cases} == set(KINDS) and {c["nk"] for c in cases} == {1, MAX_K}
    assert {c["B"] for c in cases} == {1, 2, 3, 4, 5} and {c["Cs"] for c in cases} == {1, 3}
    # ties spill into the index bits: a tied row that needs fewer elements than share the threshold key, with index passes to run
    spill = 0
    for c in cases:
        if c["kind"] in ("equal", "levels", "zeros") and index_passes(c["T"] * c["Cs"]) >= 1:
            S, k, lengths, n_b = build(c)
            key, idx = F.rank_rule(S, k, lengths)
            keys = F.key_of(S.reshape(S.shape[0], -1))
            for b in range(S.shape[0]):
                for j in range(c["nk"]):
                    tied = int((keys[b][:n_b[b]] == key[b, j]).sum())
                    took = int((F.selected_rule(S, key, idx, j, lengths)[b] & (keys[b] == key[b, j])).sum()) if tied else 0
                    spill += 0 < took < tied
            if spill > 50:
                break
    assert spill > 50
    # every kind of k is asked for somewhere: 0, 1, n - 1, n, above n, negative, duplicates
    seen = set()
    for c in cases[:40]:
        S, k, lengths, n_b = build(c)
        for b in range(S.shape[0]):
            n = int(n_b[b])
            for v in k[b].tolist():
                seen |= {name for name, hit in (("zero", v == 0), ("one", v == 1), ("n-1", v == n - 1 and n > 1), ("n", v == n and n > 1),
                                                ("above", v > n), ("negative", v < 0)) if hit}
            if len(set(k[b].tolist())) < len(k[b]):
                seen.add("duplicate")
            if lengths is not None:
                seen |= {f"len{int(v)}" for v in lengths.tolist() if v in (0, 1)}
    assert seen >= {"zero", "one", "n-1", "n", "above", "negative", "duplicate", "len0", "len1"}, seen


# ---------------------------------------------------------------- the flag
def test_spec_parser_every_key_every_refusal_and_none():
    P = F.parse_faithfulness
    assert P(None) is None and P("") is None and P("none") is None and P(" None ") is None
    assert P("explain=sbm") == F.FaithSpec("sbm", ("evidence", "saliency", "random"), 10, "deletion", "mean", "cell", 0)
    full = P("explain=gated, attr=random+evidence, steps=31, mode=insertion, fill=zero, unit=time, seed=7")
    assert full == F.FaithSpec("gated", ("random", "evidence"), 31, "insertion", "zero", "time", 7)
    assert P("attr=saliency,explain=dnn").attributions == ("saliency",) and P(full) is full
    for bad, msg in [("explain=all", "explain"), ("steps=4", "names no explain"), ("explain=sbm,steps=0", "steps"),
                     ("explain=sbm,steps=32", "steps"), ("explain=sbm,steps=2.5", "not an integer"), ("explain=sbm,mode=both", "mode"),
                     ("explain=sbm,fill=noise", "fill"), ("explain=sbm,unit=electrode", "unit"), ("explain=sbm,seed=x", "not an integer"),
                     ("explain=sbm,seed=-1", "seed"), ("explain=sbm,attr=evidence+lime", "attributions"),
                     ("explain=sbm,attr=random+random", "attributions"), ("explain=sbm,attr=", "is not one of"),
                     ("explain=sbm,explain=dnn", "given twice"), ("explain=sbm,depth=3", "is not one of"), ("explain", "is not one of"),
                     ("explain=sbm,,steps=3", "is not one of")]:
        with pytest.raises(ValueError, match=msg):
            P(bad)
    import run
    base = ["--model", "SBM", "--data", "SYNTH"]
    assert run.build_parser().parse_args(base).faithfulness == "none"
    assert run.get_args(base + ["--faithfulness", "explain=sbm,steps=4"]).faithfulness == "explain=sbm,steps=4"
    with pytest.raises(ValueError, match="steps"):
        run.get_args(base + ["--faithfulness", "explain=sbm,steps=99"])


def test_default_none_parses_imports_and_launches_nothing(monkeypatch):
    import inspect
    import run
    import exp.experiment_classification as X
    # run.main reaches the writer through the one table of explanation flags, behind the one "flag is on" predicate
    guard = [ln for ln in inspect.getsource(run.main).splitlines() if "EXPLAIN_FLAGS" in ln or "writer(" in ln or "_flag_on(" in ln]
    assert len(guard) == 3 and "_flag_on(args, flag)" in guard[1] and "!= 'none'" in inspect.getsource(run._flag_on)
    assert "faithfulness" not in inspect.getsource(run.main)
    rows = [row for row in run.EXPLAIN_FLAGS if "faithfulness" in str(row[:3])]
    assert len(rows) == 1 and rows[0][0] == "faithfulness" and rows[0][1] == "utils.faithfulness.parse_faithfulness"
    assert rows[0][3] is run.write_faithfulness
    assert not run._flag_on(run.build_parser().parse_args(["--model", "SBM", "--data", "SYNTH"]), "faithfulness")
    assert not any(hasattr(m, n) for m in (run, X) for n in ("faithfulness_curves", "parse_faithfulness", "Faithfulness"))
    monkeypatch.delitem(sys.modules, "utils.faithfulness")
    run.check_args(run.build_parser().parse_args(["--model", "SBM", "--data", "SYNTH"]))
    assert "utils.faithfulness" not in sys.modules                                      # not even the parser was imported
    monkeypatch.setitem(sys.modules, "utils.faithfulness", F)


# ---------------------------------------------------------------- ABI
def test_new_symbols_are_declared_bound_listed_and_exported():
    from ign_hip import _lib, ops
    assert _header_params(RANK) == ["score_bts", "k_bj", "len_b", "thr_key_bj", "thr_idx_bj", "B", "T", "Cs", "nk", "stream"]
    assert _header_params(PERTURB) == ["x_btc", "score_bts", "thr_key_bj", "thr_idx_bj", "j", "nk", "fill_bc", "len_b", "out_btc", "insert",
                                       "B", "T", "C", "Cs", "stream"]
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES[RANK] == (ci, [vp] * 5 + [ci] * 4 + [vp])
    assert _lib.SIGNATURES[PERTURB] == (ci, [vp] * 4 + [ci, ci] + [vp] * 3 + [ci] * 5 + [vp])
    m = re.search(r"#define\s+IGN_RANK_MAX_K\s+(\d+)", _header())
    assert m and int(m.group(1)) == ops.RANK_MAX_K == MAX_K == F.MAX_STEPS + 1
    assert re.search(r"#define\s+IGN_ABI_VERSION\s+1\b", _header())
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"`{RANK}`" in doc and f"`{PERTURB}`" in doc
    assert callable(ops.rank_threshold) and callable(ops.perturb)
    _lib_or_skip()
    h = ctypes.CDLL(_lib.lib_path())
    assert hasattr(h, RANK) and hasattr(h, PERTURB)


def test_entry_points_refuse_bad_arguments_without_a_device():
    """every refusal returns before a launch: the pointers are not device memory and no GPU is needed to run this"""
    h = _lib_or_skip().lib()
    q, o = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)

    def rank(score=q, k=q, key=q, idx=q, B=2, T=5, Cs=3, nk=4):
        return h.ign_rank_threshold(score, k, None, key, idx, B, T, Cs, nk, None)

    for kw in (dict(score=None), dict(k=None), dict(key=None), dict(idx=None), dict(B=0), dict(T=0), dict(Cs=0), dict(nk=0),
               dict(nk=MAX_K + 1)):
        assert rank(**kw) == E_ARG, kw
        assert b"ign_rank_threshold" in h.ign_last_error()
    assert rank(T=1 << 20, Cs=1 << 11) == E_TOOBIG

    def perturb(x=q, score=q, key=q, idx=q, j=1, nk=4, out=o, B=2, T=5, C=3, Cs=3):
        return h.ign_perturb_btc(x, score, key, idx, j, nk, None, None, out, 0, B, T, C, Cs, None)

    for kw in (dict(x=None), dict(score=None), dict(key=None), dict(idx=None), dict(out=None), dict(B=0), dict(T=0), dict(C=0),
               dict(Cs=0), dict(Cs=2), dict(nk=0), dict(nk=MAX_K + 1), dict(j=-1), dict(j=4), dict(out=q),
               dict(out=ctypes.c_void_p((1 << 20) + 2 * 5 * 3 * 4 - 4)), dict(x=ctypes.c_void_p((1 << 30) + 4))):
        assert perturb(**kw) == E_ARG, kw
        assert b"ign_perturb_btc" in h.ign_last_error()
    assert perturb(T=1 << 20, C=1 << 11, Cs=1) == E_TOOBIG


def test_ops_refuse_cpu_tensors_without_a_device():
    import torch
    from ign_hip import _lib, ops
    with pytest.raises(_lib.IgnError, match="rank_threshold: score must be a tensor on the GPU"):
        ops.rank_threshold(torch.zeros(2, 3, 1), torch.zeros(2, 1, dtype=torch.int32))
    with pytest.raises(_lib.IgnError, match="perturb: x must be a tensor on the GPU"):
        ops.perturb(torch.zeros(2, 3, 1), torch.zeros(2, 3, 1), torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), 0)


# ---------------------------------------------------------------- wiring against recording stand-ins
class _Rec:
    def __init__(self):
        self.log = []


def _stand_ins(monkeypatch, rec, steps):
    """ops.rank_threshold / ops.perturb that record and answer with the numpy rule on the CPU; evidence_map / input_saliency that
    record and return a fixed map"""
    import torch
    from ign_hip import ops
    from utils import evidence, saliency

    def rank(score, k, lengths=None):
        rec.log.append(("rank", tuple(score.shape), k.clone(), None if lengths is None else lengths.clone()))
        key, idx = F.rank_rule(score.numpy(), k.numpy(), None if lengths is None else lengths.numpy())
        return torch.from_numpy(key.view(np.int32).copy()), torch.from_numpy(idx)

    def perturb(x, score, thr_key, thr_idx, j, fill=None, insert=False, lengths=None):
        rec.log.append(("perturb", j, fill is not None, insert))
        return torch.from_numpy(F.perturb_rule(x.numpy(), score.numpy(), thr_key.numpy(), thr_idx.numpy(), j,
                                               None if fill is None else fill.numpy(), insert,
                                               None if lengths is None else lengths.numpy()))

    def evidence_map(model, x, target=None, explain="sbm", gating_value=None, mask=None):
        rec.log.append(("evidence", target.clone(), explain))
        return evidence.Evidence(sbm=x.abs(), target=target)

    def input_saliency(model, x, target=None, explain="sbm", gating_value=None):
        rec.log.append(("saliency", target.clone(), explain))
        return -x

    monkeypatch.setattr(ops, "rank_threshold", rank)
    monkeypatch.setattr(ops, "perturb", perturb)
    monkeypatch.setattr(evidence, "evidence_map", evidence_map)
    monkeypatch.setattr(saliency, "input_saliency", input_saliency)


def _fake_sbm(rec, **kw):
    """a CPU ShapeBottleneckModel whose forward is a fixed linear read-out of the batch, recorded"""
    import torch
    from models.Shapelet import ShapeBottleneckModel
    model = ShapeBottleneckModel(make_cfg(enc_in=2, seq_len=12, num_class=3, **kw))
    W = torch.randn(3, 24, generator=torch.Generator().manual_seed(0))

    def forward(x, *args, **kwargs):
        rec.log.append(("forward", x.clone(), model.training))
        return x.reshape(x.shape[0], -1) @ W.t(), None

    model.forward = forward
    return model, W


def test_curves_wiring_launch_counts_target_and_flags(monkeypatch):
    import torch
    rec, steps = _Rec(), 4
    _stand_ins(monkeypatch, rec, steps)
    model, W = _fake_sbm(rec)
    model.train()
    model.shapelets[1].eval()
    flags = [m.training for m in model.modules()]
    x = torch.randn(5, 12, 2, generator=torch.Generator().manual_seed(1))
    f = F.faithfulness_curves(model, x, steps=steps, fill="zero")
    assert [m.training for m in model.modules()] == flags                               # module flags restored
    kinds = [e[0] for e in rec.log]
    assert kinds[0] == "forward" and kinds.index("forward") < min(kinds.index("rank"), kinds.index("perturb"))
    logits0 = x.reshape(5, -1) @ W.t()
    assert torch.equal(f.target, logits0.argmax(1))                                     # fixed by the unperturbed forward
    assert all(torch.equal(e[1], f.target) for e in rec.log if e[0] in ("evidence", "saliency"))
    assert kinds.count("rank") == 3 and kinds.count("perturb") == 3 * (steps + 1) and kinds.count("forward") == 1 + 3 * (steps + 1)
    assert kinds.count("evidence") == 1 and kinds.count("saliency") == 1
    assert all(e[2] is False for e in rec.log if e[0] == "forward")                     # eval mode in every forward
    for e in rec.log:
        if e[0] == "rank":
            assert e[1] == (5, 12, 2) and e[3] is None
            assert e[2].tolist() == [[(j * 24) // steps for j in range(steps + 1)]] * 5 and e[2].dtype == torch.int32
        if e[0] == "perturb":
            assert e[2] is False and e[3] is False                                      # fill="zero" passes no fill; deletion
    assert [e[1] for e in rec.log if e[0] == "perturb"] == list(range(steps + 1)) * 3
    assert list(f.logit) == ["evidence", "saliency", "random"] and f.fractions.tolist() == [0, 0.25, 0.5, 0.75, 1.0]
    for a in f.logit:
        assert f.logit[a].shape == f.prob[a].shape == (steps + 1, 5) and f.flip_at[a].shape == (5,)
        assert torch.equal(f.logit[a][0], logits0.gather(1, f.target[:, None]).squeeze(1))          # fraction 0: the batch itself
        assert torch.equal(f.logit[a][steps], torch.zeros(5))                                        # everything replaced by 0
        m = f.prob[a].double().mean(1)
        assert f.auc[a] == pytest.approx(float(((m[1:] + m[:-1]) / 2).sum() / steps), abs=1e-12)
        assert f.aopc[a] == pytest.approx(float((f.logit[a][:1].double() - f.logit[a][1:].double()).mean()), abs=1e-12)
        left = (f.flip_at[a] * steps).round().long()
        assert ((left >= 0) & (left <= steps)).all() and f.flip[a] == pytest.approx(float(f.flip_at[a].mean()))
        assert f.gap[a] == pytest.approx(f.auc["random"] - f.auc[a], abs=1e-12)
    assert f.gap["random"] == 0.0
    # the random ranking is reproducible from the seed and changes with it
    rec.log.clear()
    g = F.faithfulness_curves(model, x, steps=steps, fill="zero", attributions=("random",), seed=0)
    h = F.faithfulness_curves(model, x, steps=steps, fill="zero", attributions=("random",), seed=1)
    assert torch.equal(g.logit["random"], f.logit["random"]) and not torch.equal(h.logit["random"], g.logit["random"])
    assert g.gap == {"random": 0.0} and [e[0] for e in rec.log].count("rank") == 2


def test_curves_insertion_mean_fill_time_unit_and_mask_lengths(monkeypatch):
    import torch
    rec, steps = _Rec(), 3
    _stand_ins(monkeypatch, rec, steps)
    model, W = _fake_sbm(rec, mask_padding=True)
    x = torch.randn(4, 12, 2, generator=torch.Generator().manual_seed(2))
    lengths = torch.tensor([12, 5, 0, 7])
    mask = (torch.arange(12)[None, :] < lengths[:, None]).float()
    f = F.faithfulness_curves(model, x, mask=mask, steps=steps, mode="insertion", unit="time", attributions=("evidence", "random"),
                              target=torch.tensor([0, 1, 2, 0]))
    assert f.target.tolist() == [0, 1, 2, 0] and f.mode == "insertion"
    ranks = [e for e in rec.log if e[0] == "rank"]
    assert len(ranks) == 2 and all(e[1] == (4, 12, 1) for e in ranks)                   # summed over the electrodes
    assert all(e[3].tolist() == [12, 5, 0, 7] and e[3].dtype == torch.int32 for e in ranks)
    assert ranks[0][2].tolist() == [[(j * n) // steps for j in range(steps + 1)] for n in (12, 5, 0, 7)]
    assert all(e[2] is True and e[3] is True for e in rec.log if e[0] == "perturb")     # a fill is passed; insertion
    # insertion at fraction 1 keeps everything: the unperturbed logits; at 0 every own step is its electrode's mean over the length
    logits0 = x.reshape(4, -1) @ W.t()
    assert torch.equal(f.logit["evidence"][steps], logits0.gather(1, f.target[:, None]).squeeze(1))
    x0 = [e[1] for e in rec.log if e[0] == "forward"][1]
    assert torch.allclose(x0[1, :5], x[1, :5].mean(0).expand(5, 2), atol=1e-6) and torch.equal(x0[1, 5:], x[1, 5:])
    assert torch.equal(x0[2], x[2])                                                      # an empty sample is copied through
    assert f.gap["evidence"] == pytest.approx(f.auc["evidence"] - f.auc["random"], abs=1e-12)
    with pytest.raises(ValueError, match="steps"):
        F.faithfulness_curves(model, x, steps=32)
    with pytest.raises(ValueError, match="attributions"):
        F.faithfulness_curves(model, x, attributions=())


def test_dispatch_refusals_are_those_of_evidence_map():
    import torch
    from models.InterpGN import InterpGN
    from models.Shapelet import ShapeBottleneckModel
    x = torch.zeros(2, 100, 6)
    for cls in ("bilinear", "attention"):
        with pytest.raises(ValueError, match="not additive"):
            F.faithfulness_curves(ShapeBottleneckModel(make_cfg(sbm_cls=cls)), x)
    with pytest.raises(TypeError, match="faithfulness_curves"):
        F.faithfulness_curves(torch.nn.Linear(2, 2), x)
    with pytest.raises(TypeError, match="FCN"):
        F.faithfulness_curves(ShapeBottleneckModel(make_cfg()), x, explain="dnn")
    with pytest.raises(TypeError, match="FCN is the supported deep expert"):
        F.faithfulness_curves(InterpGN(make_cfg(dnn_type="ResNet")), x, explain="gated")
    with pytest.raises(ValueError, match="explain"):
        F.faithfulness_curves(ShapeBottleneckModel(make_cfg()), x, explain="all")


def test_experiment_concatenates_and_the_writers(monkeypatch, tmp_path, capsys):
    import torch
    import run
    from argparse import Namespace
    from exp.experiment_classification import Experiment
    rec, steps = _Rec(), 2
    _stand_ins(monkeypatch, rec, steps)
    model, _ = _fake_sbm(rec)
    gen = torch.Generator().manual_seed(3)
    batches = [(torch.randn(n, 12, 2, generator=gen), torch.zeros(n, dtype=torch.long), torch.ones(n, 12)) for n in (3, 0, 2)]
    exp = Experiment.__new__(Experiment)
    exp.model, exp.test_loader, exp.args = model, batches, Namespace(gating_value=None)
    exp._to_device = lambda x, y, m: (x, y, m)
    spec = F.parse_faithfulness("explain=sbm,attr=evidence+random,steps=2,fill=zero,seed=5")
    f = exp.faithfulness(**spec._asdict())
    assert f.target.shape == (5,) and f.logit["evidence"].shape == (steps + 1, 5) and f.flip_at["random"].shape == (5,)
    whole = F.faithfulness_curves(model, batches[0][0], **dict(spec._asdict(), seed=5))
    assert torch.equal(f.logit["random"][:, :3], whole.logit["random"])                  # batch i is seeded with seed + i
    m = f.prob["evidence"].double().mean(1)
    assert f.auc["evidence"] == pytest.approx(float(((m[1:] + m[:-1]) / 2).sum() / steps), abs=1e-12)      # over all samples
    run.write_faithfulness(exp, "explain=sbm,attr=evidence+random,steps=2,fill=zero,seed=5", str(tmp_path))
    assert "faithfulness (sbm, deletion, 5 samples)" in capsys.readouterr().out
    doc = json.load(open(tmp_path / "faithfulness.json"))
    assert doc["spec"] == dict(explain="sbm", attributions=["evidence", "random"], steps=2, mode="deletion", fill="zero", unit="cell",
                               seed=5)
    assert doc["samples"] == 5 and doc["fractions"] == [0.0, 0.5, 1.0] and set(doc["auc"]) == {"evidence", "random"}
    assert all(len(doc[key][a]) == steps + 1 for key in ("mean_logit", "mean_prob") for a in ("evidence", "random"))
    assert set(doc) == {"spec", "samples", "fractions", "mean_logit", "mean_prob", "auc", "aopc", "flip", "gap"}
    z = dict(np.load(tmp_path / "faithfulness.npz"))
    assert set(z) == {"fractions", "target", "logit_evidence", "prob_evidence", "flip_at_evidence", "logit_random", "prob_random",
                      "flip_at_random"}
    assert z["logit_evidence"].shape == (steps + 1, 5) and np.array_equal(z["logit_random"], f.logit["random"].numpy())
