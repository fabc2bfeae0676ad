"""Occlusion maps on the host (no GPU): the numpy rules of utils/occlusion.py against a loop-per-cell restatement, bit for bit, on the
case table of tests/occlusion_cases.py; the coverage properties of the time grid; the --occlusion parser; the ABI of the two entry
points and their refusals, which return before any launch; the wiring of occlusion_map / Experiment.occlusion / run.py and of the
"occlusion" attribution of the faithfulness curves against recording stand-ins that answer with the numpy rule on the CPU.  The GPU
side is tests/test_gpu_occlusion.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, make_cfg
from occlusion_cases import (GRIDS, MAX_COVER, build, chunk_edges, grid_of, make_drop, make_gid, occlude_loops, occlusion_cases,
                             same_bits, spread_loops)

import speech_imagery_eeg_amd  # noqa: F401
from utils import occlusion as O

OCCLUDE, SPREAD = "ign_occlude_btc", "ign_occlusion_spread"
E_ARG, E_TOOBIG = -1001, -1003
CASES = occlusion_cases()


def _id(c):
    return f"T{c['T']}w{c['window']}s{c['stride']}-C{c['C']}-{c['groups']}-B{c['B']}{'-ragged' if c['ragged'] else ''}{'-fill' if c['fill'] else ''}"


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
def test_case_table_covers_what_it_says():
    assert {(c["T"], c["window"], c["stride"]) for c in CASES} == set(GRIDS)
    assert {c["C"] for c in CASES} == {1, 3, 5, 64, 65, 130} and {c["B"] for c in CASES} == {1, 2, 3, 4, 5}
    assert {(c["groups"], c["ragged"], c["fill"]) for c in CASES} == {(g, r, f) for g in ("all", "each", "irregular")
                                                                      for r in (False, True) for f in (False, True)}
    assert grid_of(12, 20, 4) == (12, 4, 1) and grid_of(37, 8, 3) == (8, 3, 11) and (37 - 8) % 3 != 0
    assert -(-64 // 1) == MAX_COVER == O.MAX_COVER and grid_of(129, 64, 1) == (64, 1, 66)
    for C in (3, 5, 64, 65, 130):
        gid, G = make_gid("irregular", C)
        counts = np.bincount(gid, minlength=G)
        assert (counts == 0).any() and (counts == 1).any() and gid.max() < G        # an empty group id, a group of one electrode


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_rules_equal_the_loop_restatement_bit_for_bit(case):
    x, gid, G, lengths, fill = build(case)
    B, T, C = x.shape
    window, stride = case["window"], case["stride"]
    W, S, nt = O.grid(T, window, stride)
    assert (W, S, nt) == grid_of(T, window, stride)
    P = nt * G
    n = np.full(B, T) if lengths is None else np.clip(lengths, 0, T)
    for p0, count in chunk_edges(P):
        got = O.occlude_rule(x, p0, count, gid, G, window, stride, fill=fill, lengths=lengths)
        assert got.dtype == np.float32 and got.shape == (B * count, T, C)
        assert same_bits(got, occlude_loops(x, p0, count, gid, G, window, stride, fill=fill, lengths=lengths)), (p0, count)
        for b in range(B):
            for q in range(count):
                i, g = divmod(p0 + q, G)
                if i * S >= n[b] or not (gid == g).any():                            # beyond the length / an empty group: a copy
                    assert same_bits(got[b * count + q], x[b])
    drop = make_drop(B, P, case["seed"])
    m = O.spread_rule(drop, gid, G, window, stride, T, lengths=lengths)
    assert m.dtype == np.float32 and m.shape == (B, T, C)
    assert same_bits(m, spread_loops(drop, gid, G, window, stride, T, lengths=lengths))
    outside = np.arange(T)[None, :] >= n[:, None]
    assert (m.view(np.uint32)[outside] == 0).all()                                     # +0.0 beyond the length
    if case["groups"] == "all":
        assert (m.view(np.uint32) == m.view(np.uint32)[:, :, :1]).all()               # time-only: constant across electrodes


def test_fill_none_is_a_zero_fill_and_nan_payloads_survive():
    x, gid, G, lengths, fill = build(dict(T=12, window=5, stride=2, C=5, groups="irregular", B=4, ragged=True, fill=True, seed=7))
    a = O.occlude_rule(x, 0, 3, gid, G, 5, 2, lengths=lengths)
    b = O.occlude_rule(x, 0, 3, gid, G, 5, 2, fill=np.zeros((4, 5), np.float32), lengths=lengths)
    assert same_bits(a, b)
    x[:] = 1.0
    full = O.occlude_rule(x, 0, 4, gid, G, 0, 0, fill=fill)                            # window 0: the whole series, one copy per group
    bits = full.view(np.uint32)
    assert gid.tolist() == [0, 3, 3, 0, 2] and bits.shape == (16, 12, 5)
    assert (bits[0, :, 0] == 0x80000000).all() and (bits[0, :, 1] == 0x3f800000).all()             # sample 0, group 0: -0.0 put in
    assert same_bits(full[1], x[0])                                                                  # group 1 has no electrode
    assert (bits[3, :, 1] == 0x7fc00123).all() and (bits[3, :, 2] == 0x7f800000).all() and (bits[3, :, 0] == 0x3f800000).all()


@pytest.mark.parametrize("T", [1, 2, 3, 7, 12, 37, 64, 65, 1000])
def test_grid_coverage_properties(T):
    pairs = [(W, S) for W in range(1, T + 1) for S in range(1, W + 1)]
    if T == 1000:
        rng = np.random.default_rng(0)
        pairs = [pairs[i] for i in rng.choice(len(pairs), 300, replace=False)] + [(1, 1), (1000, 1), (1000, 1000), (999, 998), (64, 1)]
    t = np.arange(T)
    for W, S in pairs:
        assert O.grid(T, W, S) == grid_of(T, W, S)
        nt = grid_of(T, W, S)[2]
        assert (nt - 1) * S < T and (nt == 1 or (nt - 2) * S + W < T)                  # the last window starts inside; none is spare
        i = np.arange(nt)
        over = (i[None, :] * S <= t[:, None]) & (t[:, None] < i[None, :] * S + W)      # (T, nt), brute force
        cnt = over.sum(1)
        assert cnt.min() >= 1 and cnt.max() <= -(-W // S)
        lo, hi = O.cover_range(T, W, S, nt)
        assert np.array_equal(lo, over.argmax(1)) and np.array_equal(hi, nt - 1 - over[:, ::-1].argmax(1))
        assert np.array_equal(cnt, hi - lo + 1)                                        # the covering windows are consecutive
    assert O.grid(T, 0, 0) == (T, T, 1) and O.grid(T, T + 5, 0) == (T, T, 1)
    with pytest.raises(ValueError, match="uncovered"):
        O.grid(T, 1, 2)
    with pytest.raises(ValueError, match="uncovered"):
        O.grid(max(T, 2), 0, max(T, 2) + 1)


def test_a_constant_drop_spreads_to_that_constant_inside_every_length():
    """The mean of k equal terms is fl(fl(k c) * inv[k]).  For c a power of two the sum is exact and the product rounds to c exactly
    where k * inv[k] rounds to 1 in float32 -- every k <= 64 but 41, 47, 55 and 61, where the rounded reciprocal is short enough of
    1 / k for the product to land on the float below c: a property of the host's table, derived below without the rule.  There the
    map is that neighbour, 2^-24 |c| away."""
    k = np.arange(1, MAX_COVER + 1, dtype=np.float32)
    inv = np.float32(1.0) / k
    off = [int(v) for v in k[(k * inv).astype(np.float32) != 1.0]]
    assert off == [41, 47, 55, 61] and np.array_equal(O.inv_table(MAX_COVER)[1:], inv) and O.inv_table(3)[0] == 0.0
    for T, window, stride in GRIDS:
        W, S, nt = grid_of(T, window, stride)
        lo, hi = O.cover_range(T, W, S, nt)
        exact = ~np.isin(hi - lo + 1, off)
        for kind in ("all", "irregular"):
            gid, G = make_gid(kind, 5)
            lengths = np.array([T, 0, 1, (T + 1) // 2], np.int32)
            for c in (1.0, -2.0, 0.25):
                m = O.spread_rule(np.full((4, nt * G), c, np.float32), gid, G, window, stride, T, lengths=lengths)
                for b in range(4):
                    n = min(int(lengths[b]), T)
                    assert (m[b, :n][exact[:n]] == np.float32(c)).all() and (m.view(np.uint32)[b, n:] == 0).all()
                    near = np.abs(m[b, :n].astype(np.float64) - c) <= abs(c) * 2.0 ** -24          # one unit below |c|, a power of two
                    assert near.all()
    assert not exact.all()                                                             # (129, 64, 1) reaches those counts


# ---------------------------------------------------------------- the flag
def test_spec_parser_every_key_every_refusal_and_none():
    P = O.parse_occlusion
    assert P(None) is None and P("") is None and P("none") is None and P(" None ") is None
    assert P("explain=model") == O.OccSpec("model", 0, 0, "all", "mean", "logit", 256)
    full = P("explain=sbm, window=8, stride=4, groups=each, fill=zero, score=prob, rows=64")
    assert full == O.OccSpec("sbm", 8, 4, "each", "zero", "prob", 64) and P(full) is full
    assert P("groups=regions.npy,explain=gated").groups == "regions.npy" and P("explain=dnn,stride=3").stride == 3
    for bad, msg in [("explain=all", "explain"), ("window=4", "names no explain"), ("explain=sbm,window=-1", "window"),
                     ("explain=sbm,window=2.5", "not an integer"), ("explain=sbm,stride=-2", "stride"),
                     ("explain=sbm,window=4,stride=5", "uncovered"), ("explain=sbm,groups=pairs", "groups"),
                     ("explain=sbm,fill=noise", "fill"), ("explain=sbm,score=loss", "score"), ("explain=sbm,rows=0", "rows"),
                     ("explain=sbm,rows=x", "not an integer"), ("explain=sbm,explain=dnn", "given twice"),
                     ("explain=sbm,depth=3", "is not one of"), ("explain", "is not one of"), ("explain=sbm,,rows=3", "is not one of"),
                     ("explain=sbm,groups=", "is not one of")]:
        with pytest.raises(ValueError, match=msg):
            P(bad)
    import run
    base = ["--model", "SBM", "--data", "SYNTH"]
    assert run.build_parser().parse_args(base).occlusion == "none"
    assert run.get_args(base + ["--occlusion", "explain=sbm,window=8"]).occlusion == "explain=sbm,window=8"
    with pytest.raises(ValueError, match="uncovered"):
        run.get_args(base + ["--occlusion", "explain=sbm,window=2,stride=3"])
    with pytest.raises(ValueError, match="regression"):
        run.check_args(run.build_parser().parse_args(base + ["--occlusion", "explain=model", "--task_name", "regression"]))


def test_the_faithfulness_flag_gains_the_model_and_the_occlusion_grid():
    from utils import faithfulness as F
    P = F.parse_faithfulness
    assert F.ATTRIBUTIONS == ("evidence", "saliency", "random") and set(F.ALLOWED_ATTRIBUTIONS) == set(F.ATTRIBUTIONS) | {"occlusion"}
    assert P("explain=sbm") == F.FaithSpec("sbm", ("evidence", "saliency", "random"), 10, "deletion", "mean", "cell", 0)
    got = P("explain=model,attr=occlusion+random,window=8,stride=4,groups=each,steps=5")
    assert got == F.FaithSpec("model", ("occlusion", "random"), 5, "deletion", "mean", "cell", 0, 8, 4, "each")
    assert P("explain=gated,attr=evidence+occlusion").attributions == ("evidence", "occlusion")
    for bad, msg in [("explain=model", "attributions"), ("explain=model,attr=evidence+random", "attributions"),
                     ("explain=model,attr=saliency", "attributions"), ("explain=sbm,attr=occlusion,window=3,stride=4", "uncovered"),
                     ("explain=sbm,attr=occlusion,groups=pairs", "groups"), ("explain=sbm,attr=occlusion,window=-1", "window")]:
        with pytest.raises(ValueError, match=msg):
            P(bad)
    spec = P("explain=sbm,attr=evidence+random")
    assert set(spec._asdict()) == {"explain", "attributions", "steps", "mode", "fill", "unit", "seed", "window", "stride", "groups"}


def test_default_none_parses_imports_and_launches_nothing(monkeypatch):
    import inspect
    import run
    import exp.experiment_classification as X
    # run.main reaches the writer through the one table of explanation flags, behind the one "flag is on" predicate
    guard = [ln for ln in inspect.getsource(run.main).splitlines() if "EXPLAIN_FLAGS" in ln or "writer(" in ln or "_flag_on(" in ln]
    assert len(guard) == 3 and "_flag_on(args, flag)" in guard[1] and "!= 'none'" in inspect.getsource(run._flag_on)
    assert "occlusion" not in inspect.getsource(run.main)
    rows = [row for row in run.EXPLAIN_FLAGS if "occlusion" in str(row[:3])]
    assert len(rows) == 1 and rows[0][0] == "occlusion" and rows[0][1] == "utils.occlusion.parse_occlusion"
    assert "write_occlusion(" in inspect.getsource(rows[0][3])
    assert not run._flag_on(run.build_parser().parse_args(["--model", "SBM", "--data", "SYNTH"]), "occlusion")
    assert not any(hasattr(m, n) for m in (run, X) for n in ("occlusion_map", "parse_occlusion", "Occlusion"))
    monkeypatch.delitem(sys.modules, "utils.occlusion")
    run.check_args(run.build_parser().parse_args(["--model", "SBM", "--data", "SYNTH"]))
    assert "utils.occlusion" not in sys.modules                                         # not even the parser was imported
    monkeypatch.setitem(sys.modules, "utils.occlusion", O)


def test_the_parser_imports_without_torch():
    import subprocess
    code = ("import sys; sys.modules['torch'] = None; sys.path.insert(0, sys.argv[1]); from utils.occlusion import parse_occlusion; "
            "print(parse_occlusion('explain=model,window=4').window)")
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "speech-imagery-eeg_amd")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "4", out.stderr


# ---------------------------------------------------------------- ABI
def test_new_symbols_are_declared_bound_listed_and_exported():
    from ign_hip import _lib, ops
    assert _header_params(OCCLUDE) == ["x_btc", "fill_bc", "len_b", "gid_c", "out", "p0", "Pc", "G", "W", "S", "nt", "B", "T", "C", "stream"]
    assert _header_params(SPREAD) == ["drop_bp", "gid_c", "len_b", "inv_k", "out_btc", "G", "W", "S", "nt", "B", "T", "C", "stream"]
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES[OCCLUDE] == (ci, [vp] * 5 + [ci] * 9 + [vp])
    assert _lib.SIGNATURES[SPREAD] == (ci, [vp] * 5 + [ci] * 7 + [vp])
    m = re.search(r"#define\s+IGN_OCC_MAX_COVER\s+(\d+)", _header())
    assert m and int(m.group(1)) == ops.OCC_MAX_COVER == MAX_COVER == O.MAX_COVER
    assert re.search(r"#define\s+IGN_ABI_VERSION\s+1\b", _header())
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"`{OCCLUDE}`" in doc and f"`{SPREAD}`" in doc
    assert callable(ops.occlude) and callable(ops.occlusion_spread)
    _lib_or_skip()
    h = ctypes.CDLL(_lib.lib_path())
    assert hasattr(h, OCCLUDE) and hasattr(h, SPREAD)


def test_entry_points_refuse_bad_arguments_without_a_device():
    """every refusal returns before a launch: the pointers are not device memory and no GPU is needed to run this"""
    h = _lib_or_skip().lib()
    q, g, o = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24), ctypes.c_void_p(1 << 30)

    def occlude(x=q, gid=g, out=o, p0=0, Pc=2, G=3, W=4, S=2, nt=3, B=2, T=7, C=3):
        return h.ign_occlude_btc(x, None, None, gid, out, p0, Pc, G, W, S, nt, B, T, C, None)

    xbytes = 2 * 7 * 3 * 4
    for kw in (dict(x=None), dict(gid=None), dict(out=None), dict(B=0), dict(T=0), dict(C=-1), dict(G=0), dict(S=0), dict(S=5),
               dict(W=8, nt=1), dict(nt=2), dict(nt=4), dict(p0=-1), dict(Pc=0), dict(p0=8), dict(p0=7, Pc=3), dict(out=q),
               dict(out=ctypes.c_void_p((1 << 20) + xbytes - 4)), dict(x=ctypes.c_void_p((1 << 30) + 2 * xbytes - 4))):
        assert occlude(**kw) == E_ARG, kw
        assert OCCLUDE.encode() in h.ign_last_error(), kw
    assert occlude(T=1 << 20, C=1 << 11, W=1, S=1, nt=1 << 20) == E_TOOBIG and OCCLUDE.encode() in h.ign_last_error()
    assert occlude(B=1 << 10, Pc=1 << 10, G=1 << 10, T=1 << 10, W=1, S=1, nt=1 << 10, C=2) == E_TOOBIG    # B*Pc*T*C = 2^31

    def spread(drop=q, gid=g, inv=g, out=o, G=3, W=4, S=2, nt=3, B=2, T=7, C=3):
        return h.ign_occlusion_spread(drop, gid, None, inv, out, G, W, S, nt, B, T, C, None)

    for kw in (dict(drop=None), dict(gid=None), dict(inv=None), dict(out=None), dict(B=0), dict(T=-3), dict(C=0), dict(G=0), dict(S=0),
               dict(S=5), dict(W=8, nt=1), dict(nt=2), dict(nt=4), dict(T=200, W=130, S=2, nt=36)):
        assert spread(**kw) == E_ARG, kw
        assert SPREAD.encode() in h.ign_last_error(), kw
    assert b"IGN_OCC_MAX_COVER" in h.ign_last_error()                                    # ceil(130 / 2) = 65 windows over a step
    assert spread(T=1 << 20, C=1 << 11, W=1, S=1, nt=1 << 20) == E_TOOBIG and SPREAD.encode() in h.ign_last_error()


def test_ops_refuse_cpu_tensors_without_a_device():
    import torch
    from ign_hip import _lib, ops
    with pytest.raises(_lib.IgnError, match="occlude: x must be a tensor on the GPU"):
        ops.occlude(torch.zeros(2, 3, 1), 0, 1, np.zeros(1, np.int32), 1, 0, 0)
    with pytest.raises(_lib.IgnError, match="occlusion_spread: drop must be a tensor on the GPU"):
        ops.occlusion_spread(torch.zeros(2, 1), np.zeros(1, np.int32), 1, 0, 0, 3)


# ---------------------------------------------------------------- wiring against recording stand-ins
class _Rec:
    def __init__(self):
        self.log = []


def _np(t):
    return None if t is None else t.numpy()


def _stand_ins(monkeypatch, rec):
    """ops.occlude / ops.occlusion_spread (and the two faithfulness ops) that record and answer with the numpy rule on the CPU"""
    import torch
    from ign_hip import ops
    from utils import faithfulness as F

    def occlude(x, p0, count, gid, groups, window, stride, fill=None, lengths=None):
        rec.log.append(("occlude", p0, count, fill is not None, None if lengths is None else lengths.clone()))
        return torch.from_numpy(O.occlude_rule(x.numpy(), p0, count, gid, groups, window, stride, _np(fill), _np(lengths)))

    def spread(drop, gid, groups, window, stride, T, lengths=None):
        rec.log.append(("spread", tuple(drop.shape), T))
        return torch.from_numpy(O.spread_rule(drop.numpy(), gid, groups, window, stride, T, _np(lengths)))

    def rank(score, k, lengths=None):
        key, idx = F.rank_rule(score.numpy(), k.numpy(), _np(lengths))
        return torch.from_numpy(key.view(np.int32).copy()), torch.from_numpy(idx)

    def perturb(x, score, thr_key, thr_idx, j, fill=None, insert=False, lengths=None):
        return torch.from_numpy(F.perturb_rule(x.numpy(), score.numpy(), thr_key.numpy(), thr_idx.numpy(), j, _np(fill), insert,
                                               _np(lengths)))

    monkeypatch.setattr(ops, "occlude", occlude)
    monkeypatch.setattr(ops, "occlusion_spread", spread)
    monkeypatch.setattr(ops, "rank_threshold", rank)
    monkeypatch.setattr(ops, "perturb", perturb)


T_, C_, N_ = 12, 2, 3


def _fake_sbm(rec, W=None, **kw):
    """a CPU ShapeBottleneckModel whose forward is a fixed linear read-out of the batch, recorded"""
    import torch
    from models.Shapelet import ShapeBottleneckModel
    model = ShapeBottleneckModel(make_cfg(enc_in=C_, seq_len=T_, num_class=N_, **kw))
    if W is None:
        W = torch.randn(N_, T_ * C_, generator=torch.Generator().manual_seed(0))

    def forward(x, *args, **kwargs):
        rec.log.append(("forward", x.clone(), model.training, args[0].clone() if args and args[0] is not None else None))
        return x.reshape(x.shape[0], -1) @ W.t(), None

    model.forward = forward
    return model, W


@pytest.mark.parametrize("rows,groups", [(256, "each"), (10, "each"), (7, "all"), (1, "irregular")])
def test_map_wiring_forward_count_eval_flags_target_and_mask(monkeypatch, rows, groups):
    import torch
    rec = _Rec()
    _stand_ins(monkeypatch, rec)
    model, W = _fake_sbm(rec, mask_padding=True)
    model.train()
    model.shapelets[1].eval()
    flags = [m.training for m in model.modules()]
    B, window, stride = 5, 5, 2
    x = torch.randn(B, T_, C_, generator=torch.Generator().manual_seed(1))
    lengths = torch.tensor([12, 5, 0, 7, 12])
    mask = (torch.arange(T_)[None, :] < lengths[:, None]).float()
    gid, G = make_gid(groups, C_)
    occ = O.occlusion_map(model, x, mask=mask, explain="sbm", window=window, stride=stride, groups=gid if groups == "irregular" else groups,
                          rows=rows)
    assert [m.training for m in model.modules()] == flags                               # module flags restored
    nt = grid_of(T_, window, stride)[2]
    P, Pc = nt * G, max(1, rows // B)
    kinds = [e[0] for e in rec.log]
    assert kinds.count("forward") == 1 + -(-P // Pc) == 1 + kinds.count("occlude") and kinds.count("spread") == 1
    assert kinds[0] == "forward" and kinds[-1] == "spread"
    assert all(e[2] is False for e in rec.log if e[0] == "forward")                     # eval mode in every forward
    logits0 = x.reshape(B, -1) @ W.t()
    assert torch.equal(occ.target, logits0.argmax(1))                                   # fixed by the unperturbed forward ...
    assert torch.equal(occ.base, logits0.gather(1, occ.target[:, None]).squeeze(1))
    chunks = [(e[1], e[2]) for e in rec.log if e[0] == "occlude"]
    assert chunks == [(p0, min(Pc, P - p0)) for p0 in range(0, P, Pc)]
    assert all(e[3] is True and e[4].tolist() == [12, 5, 0, 7, 12] and e[4].dtype == torch.int32 for e in rec.log if e[0] == "occlude")
    fwd = [e for e in rec.log if e[0] == "forward"]
    assert torch.equal(fwd[0][1], x) and torch.equal(fwd[0][3], mask)
    for (p0, n), e in zip(chunks, fwd[1:]):
        assert e[1].shape == (B * n, T_, C_) and torch.equal(e[3], mask.repeat_interleave(n, dim=0))     # the mask repeated row-wise
    # ... and the drops are those of that class: the rule applied by hand
    fill = np.stack([x[b, :int(lengths[b])].mean(0).numpy() if lengths[b] else np.zeros(C_, np.float32) for b in range(B)])
    copies = O.occlude_rule(x.numpy(), 0, P, gid, G, window, stride, fill=occlusion_fill(x, lengths), lengths=lengths.numpy())
    s = torch.from_numpy(copies).reshape(B * P, -1) @ W.t()
    want = occ.base[:, None] - s.gather(1, occ.target.repeat_interleave(P)[:, None]).view(B, P)
    assert occ.drop.shape == (B, P) and torch.allclose(occ.drop, want, atol=1e-5) and np.allclose(occlusion_fill(x, lengths), fill, atol=1e-6)
    assert same_bits(occ.map.numpy(), O.spread_rule(occ.drop.numpy(), gid, G, window, stride, T_, lengths=lengths.numpy()))
    assert (occ.map[2] == 0).all() and (occ.map[1, 5:] == 0).all() and occ.map.shape == (B, T_, C_)


def occlusion_fill(x, lengths):
    import torch
    return O.mean_fill(x, lengths.to(torch.int32)).numpy()


def test_map_target_score_fill_and_refusals(monkeypatch):
    import torch
    from models.InterpGN import InterpGN
    from models.Shapelet import ShapeBottleneckModel
    rec = _Rec()
    _stand_ins(monkeypatch, rec)
    model, W = _fake_sbm(rec)
    x = torch.randn(3, T_, C_, generator=torch.Generator().manual_seed(4))
    mask = torch.ones(3, T_)
    mask[1, 6:] = 0
    occ = O.occlusion_map(model, x, mask=mask, target=torch.tensor([2, 0, 1]), explain="model", window=4, fill="zero", score="prob")
    assert occ.target.tolist() == [2, 0, 1]
    occl = [e for e in rec.log if e[0] == "occlude"]
    assert all(e[3] is False and e[4] is None for e in occl)                            # fill="zero" passes none; mask_padding off: no lengths
    p0 = torch.softmax(x.reshape(3, -1) @ W.t(), 1).gather(1, occ.target[:, None]).squeeze(1)
    assert torch.equal(occ.base, p0) and occ.drop.shape == (3, 3)
    assert O.occlusion_map(model, x, target=1, explain="sbm").target.tolist() == [1, 1, 1]
    for kw, err, msg in [(dict(explain="all"), ValueError, "explain"), (dict(window=3, stride=4), ValueError, "uncovered"),
                         (dict(window=-1), ValueError, "window"), (dict(fill="noise"), ValueError, "fill"),
                         (dict(score="loss"), ValueError, "score"), (dict(rows=0), ValueError, "rows"),
                         (dict(groups="pairs"), ValueError, "groups"), (dict(groups=np.zeros(3, np.int64)), ValueError, "groups"),
                         (dict(groups=np.array([0, -1])), ValueError, "groups"), (dict(groups=np.zeros(2)), ValueError, "groups"),
                         (dict(explain="dnn"), TypeError, "FCN"), (dict(explain="gated"), TypeError, "InterpGN")]:
        with pytest.raises(err, match=msg):
            O.occlusion_map(model, x, **kw)
    with pytest.raises(ValueError, match="more than 64"):
        O.occlusion_map(ShapeBottleneckModel(make_cfg(enc_in=2, seq_len=200)), torch.zeros(1, 200, 2), window=130, stride=2)
    with pytest.raises(TypeError, match="occlusion_map"):
        O.occlusion_map(torch.nn.Linear(2, 2), x, explain="sbm")
    with pytest.raises(TypeError, match="occlusion_map"):
        O.occlusion_map(lambda v: v, x)
    big = torch.zeros(2, 100, 6)
    with pytest.raises(TypeError, match="FCN is the supported deep expert"):
        O.occlusion_map(InterpGN(make_cfg(dnn_type="ResNet")), big, explain="gated")
    with pytest.raises(TypeError, match="FCN is the supported deep expert"):
        O.occlusion_map(InterpGN(make_cfg(dnn_type="ResNet")), big, explain="dnn")
    with pytest.raises(ValueError, match="x must be"):
        O.occlusion_map(model, x[0])


def test_model_logits_follows_the_calling_convention_of_the_experiment():
    import torch
    from models.InterpGN import InterpGN
    from models.eegcnn import EEGCNNTransformer
    seen = []

    class Bare(torch.nn.Module):                                                        # --model DNN: bare logits
        def forward(self, x, mark, dec, mark_dec):
            seen.append(("dnn", x.shape, mark, dec, mark_dec))
            return x.sum(1)

    x, mask = torch.zeros(2, 5, 3), torch.ones(2, 5)
    assert O.model_logits(Bare(), x, mask, gating_value=0.5).shape == (2, 3) and seen[-1][2] is mask and seen[-1][3] is None
    eeg = EEGCNNTransformer.__new__(EEGCNNTransformer)
    torch.nn.Module.__init__(eeg)
    eeg.forward = lambda v, *a, **k: (seen.append(("eeg", v.shape, a, k)) or (v.sum(2), None))
    assert O.model_logits(eeg, x, mask).shape == (2, 3) and seen[-1] == ("eeg", (2, 3, 5), (), {})      # (B,C,T), no mask
    ign = InterpGN.__new__(InterpGN)
    torch.nn.Module.__init__(ign)
    ign.forward = lambda v, *a, **k: (seen.append(("ign", a, k)) or (v.sum(1), "info"))
    O.model_logits(ign, x, mask, gating_value=0.5)
    assert seen[-1][1][0] is mask and seen[-1][2] == dict(gating_value=0.5)
    assert O.shapelet_expert(Bare()) is None and O.shapelet_expert(eeg) is None


def test_the_map_of_a_linear_read_out_equals_its_closed_form(monkeypatch):
    """f(x) = <W_n, x>: hiding patch p changes the logit by sum over its cells of W_n[t,c] * (x[t,c] - fill[c]); the map is the mean of
    those sums over the windows on a cell's step -- computed here in float64, cell by cell"""
    import torch
    rec = _Rec()
    _stand_ins(monkeypatch, rec)
    model, W = _fake_sbm(rec)
    B = 4
    x = torch.randn(B, T_, C_, generator=torch.Generator().manual_seed(5))
    for window, stride, groups, fill in [(5, 2, "each", "mean"), (3, 3, "all", "zero"), (0, 0, "each", "mean"), (4, 1, "all", "mean")]:
        occ = O.occlusion_map(model, x, explain="sbm", window=window, stride=stride, groups=groups, fill=fill, rows=11)
        Wd, S, nt = grid_of(T_, window, stride)
        gid, G = make_gid(groups, C_)
        xd, wd = x.double().numpy(), W.double().numpy().reshape(N_, T_, C_)
        fd = xd.mean(1) if fill == "mean" else np.zeros((B, C_))
        want = np.zeros((B, T_, C_))
        for b in range(B):
            n = int(occ.target[b])
            for t in range(T_):
                over = [i for i in range(nt) if i * S <= t < i * S + Wd]
                for c in range(C_):
                    drops = [sum(wd[n, u, e] * (xd[b, u, e] - fd[b, e]) for u in range(i * S, min(i * S + Wd, T_)) for e in range(C_)
                                 if gid[e] == gid[c]) for i in over]
                    want[b, t, c] = sum(drops) / len(drops)
        assert np.abs(occ.map.double().numpy() - want).max() <= 1e-5 * np.abs(want).max()


def test_occlusion_beats_the_random_ranking_on_a_planted_block(monkeypatch):
    import torch
    from utils import faithfulness as F
    rec = _Rec()
    _stand_ins(monkeypatch, rec)
    W = torch.zeros(N_, T_, C_)
    W[0, 4:7, 1] = 2.0                                                                  # class 0 reads three cells of electrode 1 only
    model, _ = _fake_sbm(rec, W=W.reshape(N_, -1))
    x = 1.0 + 0.1 * torch.rand(6, T_, C_, generator=torch.Generator().manual_seed(6))
    f = F.faithfulness_curves(model, x, explain="sbm", attributions=("occlusion", "random"), steps=8, fill="zero", window=1, groups="each",
                              target=0)
    assert list(f.logit) == ["occlusion", "random"] and f.mode == "deletion"
    assert f.gap["occlusion"] > 0 and f.gap["random"] == 0.0
    assert bool((f.logit["occlusion"][1] == 0).all())                                   # 3 of 24 cells go first: the planted block
    # the default request is unchanged, and the grid fields stay out of a spec file that does not use them
    spec = F.parse_faithfulness("explain=sbm,attr=evidence+random")
    assert "window" not in F.to_json(f, spec)["spec"]
    assert F.to_json(f, F.parse_faithfulness("explain=sbm,attr=occlusion+random,window=1,groups=each"))["spec"]["groups"] == "each"


def test_faithfulness_dispatch_with_the_occlusion_attribution(monkeypatch):
    import torch
    from models.InterpGN import InterpGN
    from models.Shapelet import ShapeBottleneckModel
    from utils import faithfulness as F
    x = torch.zeros(2, 100, 6)
    for cls in ("bilinear", "attention"):
        model = ShapeBottleneckModel(make_cfg(sbm_cls=cls))
        for attrs in (("evidence", "occlusion"), ("evidence",), ("saliency", "random"), F.ATTRIBUTIONS):
            with pytest.raises(ValueError, match="not additive"):
                F.faithfulness_curves(model, x, attributions=attrs)
    for attrs in (("evidence",), ("saliency", "occlusion"), F.ATTRIBUTIONS):
        with pytest.raises(ValueError, match="attributions"):
            F.faithfulness_curves(ShapeBottleneckModel(make_cfg()), x, explain="model", attributions=attrs)
    with pytest.raises(TypeError, match="FCN is the supported deep expert"):
        F.faithfulness_curves(InterpGN(make_cfg(dnn_type="ResNet")), x, explain="gated", attributions=("occlusion",))
    # accepted: a bilinear head under explain="sbm" with nothing but occlusion and random, and any model under explain="model"
    rec = _Rec()
    _stand_ins(monkeypatch, rec)
    model, _ = _fake_sbm(rec, sbm_cls="bilinear")
    xs = torch.randn(3, T_, C_, generator=torch.Generator().manual_seed(8))
    for explain in ("sbm", "model"):
        f = F.faithfulness_curves(model, xs, explain=explain, attributions=("occlusion", "random"), steps=3, window=4, stride=2)
        assert f.logit["occlusion"].shape == (4, 3) and set(f.gap) == {"occlusion", "random"}


def test_experiment_concatenates_and_the_writer(monkeypatch, tmp_path, capsys):
    import torch
    import run
    from argparse import Namespace
    from exp.experiment_classification import Experiment
    rec = _Rec()
    _stand_ins(monkeypatch, rec)
    model, _ = _fake_sbm(rec)
    gen = torch.Generator().manual_seed(3)
    batches = [(torch.randn(n, T_, C_, generator=gen), torch.zeros(n, dtype=torch.long), torch.ones(n, T_)) for n in (3, 0, 2)]
    exp = Experiment.__new__(Experiment)
    exp.model, exp.test_loader, exp.args = model, batches, Namespace(gating_value=None)
    exp._to_device = lambda x, y, m: (x, y, m)
    spec = O.parse_occlusion("explain=model,window=5,stride=2,groups=each,rows=4")
    occ = exp.occlusion(**spec._asdict())
    nt = grid_of(T_, 5, 2)[2]
    assert occ.map.shape == (5, T_, C_) and occ.drop.shape == (5, nt * C_) and occ.target.shape == occ.base.shape == (5,)
    whole = O.occlusion_map(model, batches[2][0], **spec._asdict())
    assert same_bits(occ.map[3:].numpy(), whole.map.numpy())
    assert exp.occlusion(loader=[batches[1]], **spec._asdict()).map is None             # only empty batches: every field None
    path = tmp_path / "occlusion.npz"
    run.write_occlusion(exp, "explain=model,window=5,stride=2,groups=each,rows=4", str(path))
    assert f"occlusion (model, {nt} windows x {C_} groups, 5 samples)" in capsys.readouterr().out
    z = dict(np.load(path))
    assert set(z) == {"map", "drop", "target", "base", "gid", "window", "stride", "windows", "groups"}
    assert same_bits(z["map"], occ.map.numpy()) and z["gid"].tolist() == [0, 1] and z["gid"].dtype == np.int32
    assert (int(z["window"]), int(z["stride"]), int(z["windows"]), int(z["groups"])) == (5, 2, nt, C_)
