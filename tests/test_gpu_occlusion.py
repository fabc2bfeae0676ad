"""Occlusion maps on the GPU: ign_occlude_btc and ign_occlusion_spread against the numpy rules of utils/occlusion.py bit for bit on the
case table of tests/occlusion_cases.py (every edge of the grid formula, quads that end inside a row, empty and single-electrode groups,
ragged lengths, every special bit pattern, every chunk edge), determinism, batch independence, graph capture, and
utils.occlusion.occlusion_map / faithfulness_curves(explain="model") end to end on tiny models of every family of the registry.  The
host side is tests/test_occlusion_host.py.

Every comparison is exact (integer views); there is no tolerance in this file.  The end-to-end tests compare against a restatement that
builds the copies with occlude_rule on the host, runs the same model on them with the same chunking and applies spread_rule.  No
assertion says that one attribution beats another: that is a property of a trained model, not of this code."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import make_cfg
from occlusion_cases import GRIDS, build, chunk_edges, grid_of, make_drop, make_fill, make_gid, occlusion_cases, same_bits

pytestmark = pytest.mark.gpu
GUARD = 64
CASES = occlusion_cases()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _mods():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ops
    from utils import occlusion
    return _lib, ops, occlusion


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------- the two kernels
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"T{g[0]}w{g[1]}s{g[2]}")
def test_occlude_equals_the_rule_bit_for_bit(grid):
    dev = _dev()
    _lib, ops, O = _mods()
    cases = [c for c in CASES if (c["T"], c["window"], c["stride"]) == grid]
    assert len(cases) >= 10
    for c in cases:
        x, gid, G, lengths, fill = build(c)
        B, T, C = x.shape
        W, S, nt = grid_of(*grid)
        P = nt * G
        xd, ld, fd, gd = _t(x, dev), _t(lengths, dev), _t(fill, dev), _t(gid, dev)
        ref = O.occlude_rule(x, 0, P, gid, G, grid[1], grid[2], fill=fill, lengths=lengths).reshape(B, P, T, C)
        # the entry point itself, every patch in one launch, the output inside a guarded arena
        n = B * P * T * C
        buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
        buf[:GUARD] = 12345.0
        buf[GUARD + n:] = 12345.0
        out = buf[GUARD:GUARD + n]
        _lib.check(_lib.lib().ign_occlude_btc(_p(xd), _p(fd), _p(ld), _p(gd), _p(out), 0, P, G, W, S, nt, B, T, C, _s()), "ign_occlude_btc")
        torch.cuda.synchronize()
        assert bool((buf[:GUARD] == 12345.0).all()) and bool((buf[GUARD + n:] == 12345.0).all()), c
        got = out.view(B, P, T, C).cpu().numpy()
        assert same_bits(got, ref), f"{c}: {int((got.view(np.uint32) != ref.view(np.uint32)).sum())} cells differ"
        # through the op, every chunk edge: the rows of that chunk (of the launch just checked), twice the same bits
        whole = _bits(out).view(B, P, T, C)
        for p0, count in chunk_edges(P):
            a = ops.occlude(xd, p0, count, gid, G, grid[1], grid[2], fill=fd, lengths=ld)
            b = ops.occlude(xd, p0, count, gid, G, grid[1], grid[2], fill=fd, lengths=ld)
            assert a.shape == (B * count, T, C) and torch.equal(_bits(a), _bits(b))
            assert torch.equal(_bits(a).view(B, count, T, C), whole[:, p0:p0 + count]), (c, p0, count)


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"T{g[0]}w{g[1]}s{g[2]}")
def test_spread_equals_the_rule_bit_for_bit(grid):
    dev = _dev()
    _lib, ops, O = _mods()
    for c in [c for c in CASES if (c["T"], c["window"], c["stride"]) == grid]:
        x, gid, G, lengths, _ = build(c)
        B, T, C = x.shape
        W, S, nt = grid_of(*grid)
        drop = make_drop(B, nt * G, c["seed"])
        ref = O.spread_rule(drop, gid, G, grid[1], grid[2], T, lengths=lengths)
        dd, ld, gd = _t(drop, dev), _t(lengths, dev), _t(gid, dev)
        inv = _t(O.inv_table(-(-W // S)), dev)
        n = B * T * C
        buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
        buf[:GUARD] = 12345.0
        buf[GUARD + n:] = 12345.0
        out = buf[GUARD:GUARD + n]
        _lib.check(_lib.lib().ign_occlusion_spread(_p(dd), _p(gd), _p(ld), _p(inv), _p(out), G, W, S, nt, B, T, C, _s()),
                   "ign_occlusion_spread")
        torch.cuda.synchronize()
        assert bool((buf[:GUARD] == 12345.0).all()) and bool((buf[GUARD + n:] == 12345.0).all()), c
        got = out.view(B, T, C).cpu().numpy()
        assert same_bits(got, ref), f"{c}: {int((got.view(np.uint32) != ref.view(np.uint32)).sum())} cells differ"
        a = ops.occlusion_spread(dd, gid, G, grid[1], grid[2], T, lengths=ld)
        b = ops.occlusion_spread(dd, gid, G, grid[1], grid[2], T, lengths=ld)
        assert torch.equal(_bits(a), _bits(b)) and same_bits(a.cpu().numpy(), ref)


def test_a_samples_rows_do_not_depend_on_the_batch_around_it():
    dev = _dev()
    _, ops, O = _mods()
    case = dict(T=37, window=8, stride=3, C=65, groups="irregular", B=5, ragged=True, fill=True, seed=3)
    x, gid, G, lengths, fill = build(case)
    nt = grid_of(37, 8, 3)[2]
    P = nt * G
    drop = make_drop(5, P, 9)
    xd, ld, fd, dd = _t(x, dev), _t(lengths, dev), _t(fill, dev), _t(drop, dev)
    whole = ops.occlude(xd, 2, P - 3, gid, G, 8, 3, fill=fd, lengths=ld).view(5, P - 3, 37, 65)
    spread = ops.occlusion_spread(dd, gid, G, 8, 3, 37, lengths=ld)
    for b in range(5):
        sl = slice(b, b + 1)
        alone = ops.occlude(xd[sl].contiguous(), 2, P - 3, gid, G, 8, 3, fill=fd[sl].contiguous(), lengths=ld[sl].contiguous())
        assert torch.equal(_bits(alone), _bits(whole[b])), f"sample {b} alone differs from sample {b} in the batch"
        one = ops.occlusion_spread(dd[sl].contiguous(), gid, G, 8, 3, 37, lengths=ld[sl].contiguous())
        assert torch.equal(_bits(one), _bits(spread[sl]))
    # fill=None is a zero fill
    none = ops.occlude(xd, 0, P, gid, G, 8, 3, lengths=ld)
    zero = ops.occlude(xd, 0, P, gid, G, 8, 3, fill=torch.zeros(5, 65, device=dev), lengths=ld)
    assert torch.equal(_bits(none), _bits(zero))


def test_both_launches_inside_a_graph_capture():
    """a single-branch graph: one occlude and one spread launch, replayed on new data in the same buffers"""
    dev = _dev()
    _, ops, O = _mods()
    B, T, C = 3, 50, 5
    gid, G = make_gid("irregular", C)
    nt = grid_of(T, 8, 4)[2]
    rng = np.random.default_rng(5)
    x = torch.randn(B, T, C, device=dev)
    drop = torch.randn(B, nt * G, device=dev)
    fill = _t(make_fill(B, C, 1), dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.occlude(x, 1, 7, gid, G, 8, 4, fill=fill)                                  # warm-up outside the capture: the small host
        ops.occlusion_spread(drop, gid, G, 8, 4, T)                                    # tables reach the device here, once
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.occlude(x, 1, 7, gid, G, 8, 4, fill=fill)
        m = ops.occlusion_spread(drop, gid, G, 8, 4, T)
    for _ in range(2):
        x.copy_(torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)))
        drop.copy_(torch.from_numpy(rng.standard_normal((B, nt * G)).astype(np.float32)))
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out.cpu().numpy(), O.occlude_rule(x.cpu().numpy(), 1, 7, gid, G, 8, 4, fill=fill.cpu().numpy()))
        assert same_bits(m.cpu().numpy(), O.spread_rule(drop.cpu().numpy(), gid, G, 8, 4, T))


def test_ops_refusals_launch_nothing():
    dev = _dev()
    _lib, ops, O = _mods()
    B, T, C = 2, 9, 3
    x = torch.randn(B, T, C, device=dev)
    gid = np.array([0, 1, 1], np.int32)
    E = _lib.IgnError
    for kw, msg in [(dict(x=x.cpu()), "on the GPU"), (dict(x=x.double()), "float32"), (dict(x=x.transpose(0, 1)), "contiguous"),
                    (dict(x=x.clone().requires_grad_(True)), "requires a gradient"), (dict(gid=torch.zeros(C, dtype=torch.int32, device=dev)), "host"),
                    (dict(gid=np.array([0, 1, 2], np.int32)), "gid must lie"), (dict(gid=np.array([0, -1, 1], np.int32)), "gid must lie"),
                    (dict(gid=np.zeros(4, np.int32)), "gid must be"), (dict(gid=np.zeros(3, np.float32)), "gid must be"),
                    (dict(groups=0), "gid must lie"), (dict(p0=-1), "outside"), (dict(count=0), "outside"), (dict(p0=7, count=2), "outside"),
                    (dict(fill=torch.zeros(B, C)), "on the GPU"), (dict(fill=torch.zeros(B, C + 1, device=dev)), "fill must be"),
                    (dict(lengths=torch.zeros(B, device=dev)), "lengths")]:
        a = dict(x=x, p0=0, count=2, gid=gid, groups=2, fill=None, lengths=None)
        a.update(kw)
        with pytest.raises(E, match=msg):
            ops.occlude(a["x"], a["p0"], a["count"], a["gid"], a["groups"], 4, 2, fill=a["fill"], lengths=a["lengths"])     # 4 windows x 2 groups
    with pytest.raises(ValueError, match="uncovered"):
        ops.occlude(x, 0, 1, gid, 2, 2, 3)
    nt = grid_of(T, 4, 2)[2]
    drop = torch.randn(B, nt * 2, device=dev)
    for kw, msg in [(dict(drop=drop.cpu()), "on the GPU"), (dict(drop=drop[:, :-1].contiguous()), "drop must be"),
                    (dict(drop=drop.long()), "float32"), (dict(gid=np.array([0, 2, 1], np.int32)), "gid must lie"), (dict(T=0), "time step"),
                    (dict(lengths=torch.zeros(B, dtype=torch.int64, device=dev)), "lengths")]:
        a = dict(drop=drop, gid=gid, T=T, lengths=None)
        a.update(kw)
        with pytest.raises(E, match=msg):
            ops.occlusion_spread(a["drop"], a["gid"], 2, 4, 2, a["T"], lengths=a["lengths"])
    with pytest.raises(E, match="IGN_OCC_MAX_COVER"):
        ops.occlusion_spread(torch.zeros(1, 36, device=dev), np.zeros(1, np.int32), 1, 130, 2, 200)
    assert ops.occlude(x[:0], 0, 2, gid, 2, 4, 2).shape == (0, T, C) and ops.occlusion_spread(drop[:0], gid, 2, 4, 2, T).shape == (0, T, C)


# ------------------------------------------------------------------------------------------------------------- model level
B_, T_, C_, N_ = 3, 37, 5, 3


def _x(dev, seed=1, B=B_, T=T_, C=C_):
    return torch.randn(B, T, C, generator=torch.Generator().manual_seed(seed)).to(dev)


def _model(kind, dev, **kw):
    _mods()
    from models.InterpGN import InterpGN, dnn_dict
    from models.Shapelet import DistThresholdSBM, ShapeBottleneckModel
    torch.manual_seed(0)
    cfg = make_cfg(enc_in=C_, seq_len=T_, num_class=N_, c_out=N_, dec_in=C_, **kw)
    if kind == "SBM":
        m = ShapeBottleneckModel(cfg, num_shapelet=[2, 2], shapelet_len=[0.1, 0.3])
    elif kind == "LTS":
        m = DistThresholdSBM(cfg, num_shapelet=[2, 2], shapelet_len=[0.1, 0.3])
    elif kind == "InterpGN":
        m = InterpGN(cfg, num_shapelet=[2, 2], shapelet_len=[0.1, 0.3])
    else:
        m = dnn_dict[kind](cfg)
    return m.to(dev).eval()


def _restate(O, forward, x, mask, gid, G, window, stride, fill, rows, lengths=None, score="logit"):
    """occlusion_map restated: the copies from occlude_rule on the host, the same forwards on the same chunks, spread_rule on the host
    -> (map float32 (B,T,C), drop (B,P), target, base), numpy but for the two device vectors"""
    B, T, C = x.shape
    W, S, nt = grid_of(T, window, stride)
    P = nt * G

    def pick(logits, idx):
        s = torch.softmax(logits, dim=1) if score == "prob" else logits
        return s.gather(1, idx[:, None]).squeeze(1)

    with torch.no_grad():
        logits0 = forward(x, mask).float()
        idx = logits0.argmax(1)
        base = pick(logits0, idx)
        ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=x.device)
        fill_bc = O.mean_fill(x, ln).cpu().numpy() if fill == "mean" else None
        chunk = max(1, rows // B)
        drops = []
        for p0 in range(0, P, chunk):
            n = min(chunk, P - p0)
            copies = O.occlude_rule(x.cpu().numpy(), p0, n, gid, G, window, stride, fill=fill_bc, lengths=lengths)
            logits = forward(torch.from_numpy(copies).to(x.device), None if mask is None else mask.repeat_interleave(n, dim=0)).float()
            drops.append(base[:, None] - pick(logits, idx.repeat_interleave(n)).view(B, n))
        drop = torch.cat(drops, dim=1).cpu().numpy()
    return O.spread_rule(drop, gid, G, window, stride, T, lengths=lengths), drop, idx, base


def _check_map(occ, want, B, T, C, P):
    m, drop, idx, base = want
    assert occ.map.shape == (B, T, C) and occ.drop.shape == (B, P) and occ.map.dtype == occ.drop.dtype == torch.float32
    assert torch.equal(occ.target, idx) and torch.equal(_bits(occ.base), _bits(base))
    assert same_bits(occ.drop.cpu().numpy(), drop), f"{int((occ.drop.cpu().numpy().view(np.uint32) != drop.view(np.uint32)).sum())} drops differ"
    assert same_bits(occ.map.cpu().numpy(), m)
    assert bool(torch.isfinite(occ.map).all())


MODELS = {
    "sbm-bilinear": ("SBM", dict(sbm_cls="bilinear"), "sbm"),
    "sbm-cosine": ("SBM", dict(distance_func="cosine"), "model"),
    "lts": ("LTS", dict(), "sbm"),
    "ign-resnet": ("InterpGN", dict(dnn_type="ResNet"), "model"),
    "ign-fcn-gated": ("InterpGN", dict(dnn_type="FCN"), "gated"),
    "transformer": ("Transformer", dict(), "model"),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_map_equals_the_restatement_bit_for_bit(name):
    dev = _dev()
    _, ops, O = _mods()
    kind, kw, explain = MODELS[name]
    model, x = _model(kind, dev, **kw), _x(dev)
    mask = torch.ones(B_, T_, device=dev)
    gv = 0.5 if kind == "InterpGN" else None
    if explain == "sbm":
        forward = lambda xb, m: model(xb, m)[0]
    elif kind == "InterpGN":
        forward = lambda xb, m: model(xb, m, None, None, gating_value=gv)[0]
    elif kind == "Transformer":
        forward = lambda xb, m: model(xb, m, None, None)
    else:
        forward = lambda xb, m: model(xb, m, None, None)[0]
    model.train()
    flags = [m.training for m in model.modules()]
    window, stride, rows = 8, 3, 20                                                     # 11 windows; 6 patches per forward, the last chunk short
    for groups, fill, score in (("each", "mean", "logit"), ("all", "zero", "prob")):
        gid, G = make_gid(groups, C_)
        with torch.autocast("cuda", dtype=torch.bfloat16):                              # switched off inside
            occ = O.occlusion_map(model, x, mask=mask, explain=explain, window=window, stride=stride, groups=groups, fill=fill, score=score,
                                  rows=rows, gating_value=gv)
        assert [m.training for m in model.modules()] == flags and all(p.grad is None for p in model.parameters())
        model.eval()
        _check_map(occ, _restate(O, forward, x, mask, gid, G, window, stride, fill, rows, score=score), B_, T_, C_, 11 * G)
        model.train()
        if groups == "all":
            assert bool((_bits(occ.map) == _bits(occ.map)[:, :, :1]).all())            # time-only: constant across electrodes


def test_what_the_other_explanations_refuse_is_served():
    dev = _dev()
    _lib, ops, O = _mods()
    from utils.evidence import evidence_map
    from utils.saliency import input_saliency
    x = _x(dev)
    bil = _model("SBM", dev, sbm_cls="bilinear")
    with pytest.raises(ValueError, match="not additive"):
        evidence_map(bil, x)
    cos = _model("SBM", dev, distance_func="cosine")
    with pytest.raises(_lib.IgnError):
        input_saliency(cos, x)
    res = _model("InterpGN", dev, dnn_type="ResNet")
    for explain in ("gated", "dnn"):
        with pytest.raises(TypeError, match="FCN is the supported deep expert"):
            O.occlusion_map(res, x, explain=explain)
    for model, explain in ((bil, "sbm"), (cos, "sbm"), (res, "model"), (res, "sbm")):
        occ = O.occlusion_map(model, x, explain=explain, window=0, groups="each")      # pure electrode occlusion: P = C
        assert occ.drop.shape == (B_, C_) and bool(torch.isfinite(occ.map).all())
        assert bool((_bits(occ.map) == _bits(occ.map)[:, :1, :]).all())                # ... the map is constant along time
        assert torch.equal(_bits(occ.map[:, 0, :]), _bits(occ.drop))


def test_eegcnn_at_its_shape():
    dev = _dev()
    _, ops, O = _mods()
    from models.eegcnn import EEGCNNTransformer
    torch.manual_seed(0)
    model = EEGCNNTransformer(make_cfg(enc_in=122, seq_len=1000, num_class=3, c_out=3, d_model=128)).to(dev).eval()
    x = _x(dev, seed=2, B=2, T=1000, C=122)
    occ = O.occlusion_map(model, x, mask=torch.ones(2, 1000, device=dev), window=250, stride=250, groups="all")      # the mask never reaches it
    gid, G = make_gid("all", 122)
    want = _restate(O, lambda xb, m: model(xb.permute(0, 2, 1))[0], x, None, gid, G, 250, 250, "mean", 256)
    _check_map(occ, want, 2, 1000, 122, 4)                                              # four copies per sample, one forward of 8 rows
    for i in range(4):
        blk = _bits(occ.map[:, 250 * i:250 * (i + 1)])
        assert bool((blk == blk[:, :1, :1]).all()) and torch.equal(blk[:, 0, 0], _bits(occ.drop[:, i]))


def test_ragged_batch_under_mask_padding_stays_inside_each_length():
    dev = _dev()
    _, ops, O = _mods()
    model = _model("SBM", dev, mask_padding=True, sbm_cls="attention")
    lengths = [T_, 20, 9]
    mask = (torch.arange(T_)[None, :] < torch.tensor(lengths)[:, None]).float().to(dev)
    x = _x(dev, seed=6) * mask[:, :, None]
    gid, G = make_gid("irregular", C_)
    occ = O.occlusion_map(model, x, mask=mask, explain="model", window=8, stride=3, groups=gid, rows=16)
    want = _restate(O, lambda xb, m: model(xb, m, None, None)[0], x, mask, gid, G, 8, 3, "mean", 16, lengths=np.array(lengths, np.int32))
    _check_map(occ, want, B_, T_, C_, 11 * G)
    bits = _bits(occ.map).cpu()
    for b, n in enumerate(lengths):
        assert bool((bits[b, n:] == 0).all())                                           # +0.0 beyond the length
    # a window beyond a sample's length, and a group without electrodes, hide nothing: the copy is the sample
    ln = torch.tensor(lengths, dtype=torch.int32, device=dev)
    copies = ops.occlude(x, 0, 11 * G, gid, G, 8, 3, fill=torch.full((B_, C_), 7.0, device=dev), lengths=ln).view(B_, 11, G, T_, C_)
    hit = (copies == 7.0)
    for b, n in enumerate(lengths):
        assert not bool(hit[b, :, :, n:].any()) and not bool(hit[b, :, 1].any())
        assert bool(hit[b, 0, 0, :min(8, n), 0].all())                                  # ... and the first window does hide its steps
        for i in range(11):
            if 3 * i >= n:
                assert torch.equal(_bits(copies[b, i]), _bits(x[b]).expand(G, -1, -1))


@pytest.mark.parametrize("name", ["eegcnn", "ign-resnet"])
def test_curves_for_models_without_a_built_in_explanation(name):
    dev = _dev()
    _mods()
    from utils import faithfulness as F
    if name == "eegcnn":
        from models.eegcnn import EEGCNNTransformer
        torch.manual_seed(0)
        model = EEGCNNTransformer(make_cfg(enc_in=122, seq_len=1000, num_class=3, c_out=3, d_model=128)).to(dev).eval()
        x, grid = _x(dev, seed=3, B=2, T=1000, C=122), dict(window=250, stride=250, groups="all")
        plain = lambda: model(x.permute(0, 2, 1))[0]
    else:
        model, x, grid = _model("InterpGN", dev, dnn_type="ResNet"), _x(dev), dict(window=8, stride=4, groups="each")
        plain = lambda: model(x, None, None, None, gating_value=0.5)[0]
    steps, B = 3, x.shape[0]
    f = F.faithfulness_curves(model, x, explain="model", attributions=("occlusion", "random"), steps=steps, unit="time", gating_value=0.5,
                              **grid)
    assert list(f.logit) == ["occlusion", "random"] and f.fractions.shape == (steps + 1,) and f.target.shape == (B,)
    for a in f.logit:
        assert f.logit[a].shape == f.prob[a].shape == (steps + 1, B) and f.flip_at[a].shape == (B,)
        assert bool(torch.isfinite(f.logit[a]).all()) and bool(((f.prob[a] >= 0) & (f.prob[a] <= 1)).all())
    assert set(f.gap) == {"occlusion", "random"} and f.gap["random"] == 0.0
    with torch.no_grad():
        logits = plain().float()
    assert torch.equal(f.target, logits.argmax(1))
    for a in f.logit:
        assert torch.equal(_bits(f.logit[a][0]), _bits(logits.gather(1, f.target[:, None]).squeeze(1))), a   # fraction 0: bit for bit
    with pytest.raises(ValueError, match="attributions"):
        F.faithfulness_curves(model, x, explain="model", steps=steps)                   # the default request names evidence and saliency


# ------------------------------------------------------------------------------------------------------------- driver
def test_driver_writes_occlusion_npz(tmp_path, capsys, monkeypatch):
    """run.py --occlusion on the synthetic provider (SBM with the attention head, one epoch): occlusion.npz beside the test results holds
    the maps of the whole test set and the grid; without the flag no file is written."""
    import glob
    import os
    _dev()
    _mods()
    import run
    monkeypatch.chdir(tmp_path)
    argv = ["--data", "SYNTH", "--synthetic", "24,6,100,4", "--model", "SBM", "--sbm_cls", "attention", "--train_epochs", "1",
            "--batch_size", "8", "--seed", "0", "--amp", "--log_interval", "1"]
    run.main(argv + ["--dataset", "plain"])
    assert not glob.glob(str(tmp_path / "checkpoints" / "**" / "occlusion.npz"), recursive=True)
    run.main(argv + ["--dataset", "occ", "--occlusion", "explain=sbm,window=8,stride=4,groups=each"])
    out = capsys.readouterr().out
    files = glob.glob(str(tmp_path / "checkpoints" / "**" / "occlusion.npz"), recursive=True)
    assert len(files) == 1 and "occlusion (sbm, 24 windows x 6 groups" in out, out[-2000:]
    assert os.path.exists(os.path.join(os.path.dirname(files[0]), "test_results.pkl"))
    z = dict(np.load(files[0]))
    n = z["map"].shape[0]
    assert set(z) == {"map", "drop", "target", "base", "gid", "window", "stride", "windows", "groups"} and n > 0
    assert z["map"].shape == (n, 100, 6) and z["drop"].shape == (n, 144) and z["target"].shape == z["base"].shape == (n,)
    assert z["gid"].tolist() == list(range(6)) and (int(z["window"]), int(z["stride"]), int(z["windows"]), int(z["groups"])) == (8, 4, 24, 6)
    assert np.isfinite(z["map"]).all() and same_bits(z["map"], _mods()[2].spread_rule(z["drop"], z["gid"], 6, 8, 4, 100))
