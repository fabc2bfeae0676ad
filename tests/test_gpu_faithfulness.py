"""Faithfulness curves on the GPU: ign_rank_threshold and ign_perturb_btc against the numpy rule of utils/faithfulness.py bit for bit
on the case table of tests/faithfulness_cases.py (every path of the select kernel's launch geometry, every kind of tie and bit
pattern, every edge of k, ragged lengths), determinism, batch independence, graph capture, every refusal, and
utils.faithfulness.faithfulness_curves end to end on tiny models.  The host side is tests/test_faithfulness_host.py.

Every comparison is exact (integer views); there is no tolerance in this file.  No assertion says that one attribution beats another:
that is a property of a trained model, not of this code."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import make_cfg
from faithfulness_cases import MAX_K, SIZES, TRIP, build, make_scores, rank_cases, same_bits

pytestmark = pytest.mark.gpu
GUARD = 64
SENT = 0x5a5a5a5a
E_ARG = -1001


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _mods():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ops
    from utils import faithfulness
    return _lib, ops, faithfulness


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------------------- the threshold
def _run_rank(dev, S, k, lengths):
    """One launch of the entry point with both outputs inside a sentinel-filled arena -> (thr_key uint32, thr_idx int32, arena ok)."""
    _lib, _, _ = _mods()
    B, T, Cs = S.shape
    nk = k.shape[1]
    m = B * nk
    arena = torch.full((3 * GUARD + 2 * m,), SENT, dtype=torch.int32, device=dev)
    key, idx = arena[GUARD:GUARD + m], arena[2 * GUARD + m:2 * GUARD + 2 * m]
    Sd, kd, ld = _t(S, dev), _t(k, dev), _t(lengths, dev)                          # named: alive until the launch has run
    _lib.check(_lib.lib().ign_rank_threshold(_p(Sd), _p(kd), _p(ld), _p(key), _p(idx), B, T, Cs, nk, _s()), "ign_rank_threshold")
    torch.cuda.synchronize()
    a = arena.cpu().numpy()
    guards = np.concatenate([a[:GUARD], a[GUARD + m:2 * GUARD + m], a[2 * GUARD + 2 * m:]])
    return a[GUARD:GUARD + m].reshape(B, nk).view(np.uint32), a[2 * GUARD + m:2 * GUARD + 2 * m].reshape(B, nk), bool((guards == SENT).all())


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_threshold_equals_the_rule_bit_for_bit(size):
    dev = _dev()
    _, ops, F = _mods()
    cases = [c for c in rank_cases() if (c["T"], c["Cs"]) == size]
    assert len(cases) == 10
    for c in cases:
        S, k, lengths, _ = build(c)
        ref_key, ref_idx = F.rank_rule(S, k, lengths)
        assert not (ref_key == SENT).any() and not (ref_idx == SENT).any()             # so equality shows every output was written
        key, idx, intact = _run_rank(dev, S, k, lengths)
        label = f"{c}"
        assert intact, label
        assert np.array_equal(key, ref_key), f"{label}: keys differ at {np.argwhere(key != ref_key)[:4].tolist()}"
        assert np.array_equal(idx, ref_idx), f"{label}: indices differ at {np.argwhere(idx != ref_idx)[:4].tolist()}"
    # through the op: the same bits, int32 outputs
    S, k, lengths, _ = build(cases[-1])
    got_key, got_idx = ops.rank_threshold(_t(S, dev), _t(k, dev), lengths=_t(lengths, dev))
    ref_key, ref_idx = F.rank_rule(S, k, lengths)
    assert got_key.dtype == got_idx.dtype == torch.int32
    assert np.array_equal(got_key.cpu().numpy().view(np.uint32), ref_key) and np.array_equal(got_idx.cpu().numpy(), ref_idx)


# ------------------------------------------------------------------------------------------------------------- the perturbation
PT_CHUNK = 4096             # flat indices per block of perturb_kernel
# (B, T, C): one cell; a few; odd rows; one below / above a block's chunk; several chunks with an odd tail
PERTURB_SHAPES = [(1, 1, 1), (3, 7, 5), (2, 37, 122), (4, PT_CHUNK // 3, 3), (5, PT_CHUNK // 3 + 1, 3), (3, 3001, 3)]


def _perturb_case(shape, Cs_is_C, seed):
    B, T, C = shape
    rng = np.random.default_rng(seed)
    Cs = C if Cs_is_C else 1
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    flat = x.reshape(-1).view(np.uint32)
    flat[rng.integers(0, flat.size, max(1, flat.size // 50))] = 0x7fc00123             # NaNs with a payload, copied through
    S = make_scores(("levels", "continuous", "special")[seed % 3], B, T, Cs, seed)
    lengths = np.array([T, 0, 1, (T + 1) // 2, T + 3][:B], np.int32) if seed % 2 else None
    n_b = np.full(B, T * Cs, np.int64) if lengths is None else np.clip(lengths.astype(np.int64), 0, T) * Cs
    k = np.stack([np.array([0, 1, n // 3, n - 1, n, n + 2]) for n in n_b]).astype(np.int32)
    fill = (rng.standard_normal((B, C)) + 10.0).astype(np.float32)                     # never a value of x
    return x, S, k, lengths, n_b, fill


@pytest.mark.parametrize("Cs_is_C", [True, False], ids=["per-cell", "per-step"])
@pytest.mark.parametrize("shape", PERTURB_SHAPES, ids=str)
def test_perturb_equals_the_rule_bit_for_bit(shape, Cs_is_C):
    dev = _dev()
    _lib, ops, F = _mods()
    B, T, C = shape
    for seed in (0, 1):
        x, S, k, lengths, n_b, fill = _perturb_case(shape, Cs_is_C, seed + 2 * C)
        Cs = S.shape[2]
        key, idx = F.rank_rule(S, k, lengths)
        xd, Sd, ld, fd = _t(x, dev), _t(S, dev), _t(lengths, dev), _t(fill, dev)
        kd, idd = _t(key.view(np.int32), dev), _t(idx, dev)
        xb = x.view(np.uint32)
        for j in range(k.shape[1]):
            n = B * T * C
            buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
            buf[:GUARD] = 12345.0
            buf[GUARD + n:] = 12345.0
            out = buf[GUARD:GUARD + n]
            _lib.check(_lib.lib().ign_perturb_btc(_p(xd), _p(Sd), _p(kd), _p(idd), j, k.shape[1], _p(fd), _p(ld), _p(out), 0, B, T, C, Cs,
                                                  _s()), "ign_perturb_btc")
            torch.cuda.synchronize()
            got = out.view(B, T, C).cpu().numpy()
            assert bool((buf[:GUARD] == 12345.0).all()) and bool((buf[GUARD + n:] == 12345.0).all())
            ref = F.perturb_rule(x, S, key, idx, j, fill=fill, lengths=lengths)
            assert same_bits(got, ref), f"seed {seed} j {j}: {int((got.view(np.uint32) != ref.view(np.uint32)).sum())} cells differ"
            ins = ops.perturb(xd, Sd, kd, idd, j, fill=fd, insert=True, lengths=ld).cpu().numpy()
            assert same_bits(ins, F.perturb_rule(x, S, key, idx, j, fill=fill, insert=True, lengths=lengths))
            # the number of cells replaced is exact, and deletion and insertion are complements inside each sample's length
            gz, iz = got.view(np.uint32), ins.view(np.uint32)
            kc = np.minimum(np.maximum(k[:, j], 0), n_b)
            assert ((gz != xb).sum((1, 2)) == kc * (C // Cs)).all()
            length = np.full(B, T) if lengths is None else np.clip(lengths, 0, T)
            inside = np.broadcast_to(np.arange(T)[None, :, None] < length[:, None, None], x.shape)
            assert ((gz != xb) != (iz != xb))[inside].all() and not (gz != xb)[~inside].any() and not (iz != xb)[~inside].any()
            if Cs == 1:                                                                 # a time step goes as a whole
                assert ((gz != xb).all(2) | (gz == xb).all(2)).all()
            # fill=None is a zero fill
            none = ops.perturb(xd, Sd, kd, idd, j, lengths=ld)
            zero = ops.perturb(xd, Sd, kd, idd, j, fill=torch.zeros(B, C, device=dev), lengths=ld)
            assert torch.equal(none.view(torch.int32), zero.view(torch.int32))
            assert same_bits(none.cpu().numpy(), F.perturb_rule(x, S, key, idx, j, lengths=lengths))


# ------------------------------------------------------------------------------------------------------------- determinism
def test_both_ops_are_repeatable_and_independent_of_the_batch():
    dev = _dev()
    _, ops, F = _mods()
    B, T, C = 5, TRIP // 3 + 1, 3
    for kind in ("levels", "continuous"):
        S = make_scores(kind, B, T, C, 11)
        x = np.random.default_rng(3).standard_normal((B, T, C)).astype(np.float32)
        lengths = np.array([T, 5, T - 1, 0, T // 2], np.int32)
        k = np.tile(np.array([[0, 1, 17, T, 3 * T - 1, 3 * T]], np.int32), (B, 1))
        Sd, xd, kd, ld = _t(S, dev), _t(x, dev), _t(k, dev), _t(lengths, dev)
        key, idx = ops.rank_threshold(Sd, kd, lengths=ld)
        key2, idx2 = ops.rank_threshold(Sd, kd, lengths=ld)
        assert torch.equal(key, key2) and torch.equal(idx, idx2)
        out = ops.perturb(xd, Sd, key, idx, 4, lengths=ld)
        assert torch.equal(out.view(torch.int32), ops.perturb(xd, Sd, key, idx, 4, lengths=ld).view(torch.int32))
        for b in range(B):
            sl = slice(b, b + 1)
            kb, ib = ops.rank_threshold(Sd[sl].contiguous(), kd[sl].contiguous(), lengths=ld[sl].contiguous())
            assert torch.equal(kb, key[sl]) and torch.equal(ib, idx[sl]), f"{kind}: sample {b} alone differs from sample {b} in the batch"
            ob = ops.perturb(xd[sl].contiguous(), Sd[sl].contiguous(), kb, ib, 4, lengths=ld[sl].contiguous())
            assert torch.equal(ob.view(torch.int32), out[sl].view(torch.int32))


def test_perturb_inside_a_graph_capture():
    """a single-branch graph: the one perturb launch, replayed on new data in the same buffers"""
    dev = _dev()
    _, ops, F = _mods()
    B, T, C = 3, 50, 4
    rng = np.random.default_rng(5)
    S = make_scores("levels", B, T, C, 2)
    k = np.tile(np.array([[0, 30, 200]], np.int32), (B, 1))
    x = torch.randn(B, T, C, device=dev)
    Sd, kd = _t(S, dev), _t(k, dev)
    key, idx = ops.rank_threshold(Sd, kd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.perturb(x, Sd, key, idx, 1)                                                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.perturb(x, Sd, key, idx, 1)
    for _ in range(2):
        x.copy_(torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)))
        g.replay()
        torch.cuda.synchronize()
        ref = F.perturb_rule(x.cpu().numpy(), S, key.cpu().numpy(), idx.cpu().numpy(), 1)
        assert same_bits(out.cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------------------- refusals
def test_every_refusal_launches_nothing():
    dev = _dev()
    _lib, ops, F = _mods()
    h = _lib.lib()
    B, T, C, nk = 2, 9, 3, 4
    x = torch.randn(B, T, C, device=dev)
    S = torch.randn(B, T, C, device=dev)
    S1 = torch.randn(B, T, 1, device=dev)
    k = torch.tensor([[0, 3, 9, 27]] * B, dtype=torch.int32, device=dev)
    key = torch.full((B, nk), 7, dtype=torch.int32, device=dev)
    idx = torch.full((B, nk), 7, dtype=torch.int32, device=dev)
    out = torch.full((B, T, C), 5.0, device=dev)

    def rank(score=S, kk=k, ko=key, io=idx, B=B, T=T, Cs=C, nk=nk):
        return h.ign_rank_threshold(_p(score), _p(kk), None, _p(ko), _p(io), B, T, Cs, nk, _s())

    for kw in (dict(score=None), dict(kk=None), dict(ko=None), dict(io=None), dict(B=0), dict(T=-1), dict(Cs=0), dict(nk=0),
               dict(nk=MAX_K + 1)):
        assert rank(**kw) == E_ARG and b"ign_rank_threshold" in h.ign_last_error(), kw

    def perturb(xx=x, score=S, ko=key, io=idx, j=1, nk=nk, oo=out, B=B, T=T, C=C, Cs=C):
        return h.ign_perturb_btc(_p(xx), _p(score), _p(ko), _p(io), j, nk, None, None, _p(oo), 0, B, T, C, Cs, _s())

    for kw in (dict(xx=None), dict(score=None), dict(ko=None), dict(io=None), dict(oo=None), dict(B=0), dict(T=0), dict(C=0), dict(Cs=0),
               dict(Cs=2), dict(nk=0), dict(nk=MAX_K + 1), dict(j=-1), dict(j=nk), dict(oo=x), dict(oo=x.view(-1)[1:])):
        assert perturb(**kw) == E_ARG and b"ign_perturb_btc" in h.ign_last_error(), kw
    torch.cuda.synchronize()
    assert bool((key == 7).all()) and bool((idx == 7).all()) and bool((out == 5.0).all())   # nothing was launched

    E = _lib.IgnError
    bad_rank = [
        (dict(score=S.cpu()), "on the GPU"), (dict(k=k.cpu()), "on the GPU"), (dict(score=S.double()), "float32"),
        (dict(k=k.long()), "int32"), (dict(score=S.transpose(1, 2)), "contiguous"), (dict(k=k[:, ::2]), "contiguous"),
        (dict(score=S.clone().requires_grad_(True)), "requires a gradient"), (dict(score=S[0]), "3 axes"),
        (dict(k=k[:1]), "nk in"), (dict(k=torch.zeros(B, MAX_K + 1, dtype=torch.int32, device=dev)), "nk in"),
        (dict(lengths=torch.zeros(B, dtype=torch.int64, device=dev)), "lengths"),
    ]
    for kw, msg in bad_rank:
        args = dict(score=S, k=k, lengths=None)
        args.update(kw)
        with pytest.raises(E, match=msg):
            ops.rank_threshold(args["score"], args["k"], lengths=args["lengths"])
    bad_perturb = [
        (dict(x=x.cpu()), "on the GPU"), (dict(x=x.half()), "float32"), (dict(x=x.transpose(0, 1)), "contiguous"),
        (dict(x=x.clone().requires_grad_(True)), "requires a gradient"), (dict(score=S.cpu()), "on the GPU"),
        (dict(score=torch.randn(B, T, 2, device=dev)), "score must be"), (dict(score=torch.randn(B, T + 1, C, device=dev)), "score must be"),
        (dict(thr_key=key.long()), "int32"), (dict(thr_idx=idx.float()), "int32"), (dict(thr_idx=idx[:, :2].contiguous()), "nk in"),
        (dict(thr_key=key.cpu()), "on the GPU"), (dict(j=-1), "outside"), (dict(j=nk), "outside"),
        (dict(fill=torch.zeros(B, C)), "on the GPU"), (dict(fill=torch.zeros(B, C + 1, device=dev)), "fill must be"),
        (dict(fill=torch.zeros(B, C, device=dev, dtype=torch.float64)), "float32"),
        (dict(fill=torch.zeros(B, C, device=dev, requires_grad=True)), "requires a gradient"),
        (dict(lengths=torch.zeros(B, device=dev)), "lengths"),
    ]
    for kw, msg in bad_perturb:
        args = dict(x=x, score=S, thr_key=key, thr_idx=idx, j=1, fill=None, lengths=None)
        args.update(kw)
        with pytest.raises(E, match=msg):
            ops.perturb(args["x"], args["score"], args["thr_key"], args["thr_idx"], args["j"], fill=args["fill"], lengths=args["lengths"])
    torch.cuda.synchronize()
    assert bool((key == 7).all()) and bool((idx == 7).all())
    # and what is accepted works: per-step scores broadcast over the electrodes
    tk, ti = ops.rank_threshold(S1, torch.tensor([[4]] * B, dtype=torch.int32, device=dev))
    got = ops.perturb(x, S1, tk, ti, 0)
    gone = (got == 0).all(2)
    assert gone.sum(1).tolist() == [4] * B and bool(((got == x) | gone[:, :, None]).all())
    assert torch.equal(gone, S1[..., 0] >= S1[..., 0].topk(4, dim=1).values[:, -1:])


# ------------------------------------------------------------------------------------------------------------- model level
B_, T_, C_, N_, K_, L_ = 3, 48, 2, 3, 2, 8


def _tiny_sbm(dev, **kw):
    _mods()
    from models.Shapelet import ShapeBottleneckModel
    torch.manual_seed(0)
    model = ShapeBottleneckModel(make_cfg(enc_in=C_, seq_len=T_, num_class=N_, **kw), num_shapelet=[K_], shapelet_len=[0.16])
    assert [(s.n, s.length, s.stride) for s in model.shapelets] == [(K_, L_, 1)]
    return model.to(dev).eval()


def _x(dev, seed=1, B=B_, T=T_, C=C_):
    return torch.randn(B, T, C, generator=torch.Generator().manual_seed(seed)).to(dev)


def _check_shapes(f, names, steps, B):
    assert list(f.logit) == list(names) and f.fractions.shape == (steps + 1,) and f.target.shape == (B,)
    for a in names:
        assert f.logit[a].shape == f.prob[a].shape == (steps + 1, B) and f.flip_at[a].shape == (B,)
        assert bool(torch.isfinite(f.logit[a]).all()) and bool(((f.prob[a] >= 0) & (f.prob[a] <= 1)).all())
        assert all(isinstance(d[a], float) for d in (f.auc, f.aopc, f.flip)) and 0.0 <= f.flip[a] <= 1.0
    assert set(f.gap) == (set(names) if "random" in names else set())


def test_sbm_fraction_zero_and_fraction_one_are_exact():
    dev = _dev()
    _, ops, F = _mods()
    model, x = _tiny_sbm(dev), _x(dev)
    with torch.no_grad():
        plain = model(x)[0]
        blank = model(torch.zeros_like(x))[0]
    steps = 4
    f = F.faithfulness_curves(model, x, steps=steps, fill="zero")
    _check_shapes(f, ("evidence", "saliency", "random"), steps, B_)
    assert torch.equal(f.target, plain.argmax(1))
    for a in f.logit:
        assert torch.equal(f.logit[a][0], plain.gather(1, f.target[:, None]).squeeze(1)), a          # fraction 0: bitwise
        assert torch.equal(f.logit[a][steps], blank.gather(1, f.target[:, None]).squeeze(1)), a      # fraction 1: the zero batch
        assert torch.equal(f.prob[a][0], torch.softmax(plain, 1).gather(1, f.target[:, None]).squeeze(1))
    ins = F.faithfulness_curves(model, x, steps=steps, fill="zero", mode="insertion", attributions=("evidence",), unit="time")
    assert torch.equal(ins.logit["evidence"][0], f.logit["evidence"][steps])
    assert torch.equal(ins.logit["evidence"][steps], f.logit["evidence"][0]) and ins.gap == {}
    again = F.faithfulness_curves(model, x, steps=steps, fill="zero")
    assert all(torch.equal(again.logit[a], f.logit[a]) for a in f.logit)                             # the seed fixes the random ranking


def test_evidence_ranking_deletes_exactly_the_matched_window():
    dev = _dev()
    _, ops, F = _mods()
    from utils.evidence import evidence_map
    model, x = _tiny_sbm(dev), _x(dev, seed=4)
    k_, c_, t0 = 1, 1, 17
    xn, _ = ops.instance_norm(x)                                                       # (B,C,T)
    with torch.no_grad():
        model.shapelets[0].weights[k_, c_] = xn[0, c_, t0:t0 + L_]                     # planted: sample 0 holds this shapelet at t0
        model.output_layer.weight.zero_()
        model.output_layer.weight[:, k_ * C_ + c_] = torch.tensor([1.0, 2.0, 3.0])    # the head weights that one shapelet only
        _, info = model(x)
    t = info.t[:, k_ * C_ + c_].cpu()
    assert int(t[0]) == t0 and bool((info.p[:, k_ * C_ + c_] > 0).all())
    ev = evidence_map(model, x)
    k = torch.full((B_, 1), L_, dtype=torch.int32, device=dev)
    key, idx = ops.rank_threshold(ev.sbm.contiguous(), k)
    out = ops.perturb(x, ev.sbm.contiguous(), key, idx, 0, fill=torch.full((B_, C_), 99.0, device=dev))
    want = torch.zeros(B_, T_, C_, dtype=torch.bool)
    for b in range(B_):
        want[b, int(t[b]):int(t[b]) + L_, c_] = True
    assert torch.equal((out == 99.0).cpu(), want) and torch.equal(out.cpu()[~want], x.cpu()[~want])


@pytest.mark.parametrize("explain", ["gated", "dnn"])
def test_curves_on_a_tiny_interpgn(explain):
    dev = _dev()
    _, ops, F = _mods()
    from models.InterpGN import InterpGN
    torch.manual_seed(0)
    model = InterpGN(make_cfg(enc_in=3, seq_len=40, num_class=3)).to(dev).eval()
    x = _x(dev, seed=2, B=4, T=40, C=3)
    model.train()
    flags = [m.training for m in model.modules()]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        f = F.faithfulness_curves(model, x, explain=explain, steps=3, gating_value=0.5)
    assert [m.training for m in model.modules()] == flags and all(p.grad is None for p in model.parameters())
    _check_shapes(f, ("evidence", "saliency", "random"), 3, 4)
    assert f.logit["evidence"].dtype == torch.float32
    model.eval()
    with torch.no_grad():
        out, info = model(x, None, None, None, gating_value=0.5)
    plain = out if explain == "gated" else info.dnn_preds
    assert torch.equal(f.target, plain.argmax(1))
    for a in f.logit:
        assert torch.equal(f.logit[a][0], plain.float().gather(1, f.target[:, None]).squeeze(1)), a
    t = F.faithfulness_curves(model, x, explain=explain, steps=2, unit="time", attributions=("evidence", "random"), target=1)
    _check_shapes(t, ("evidence", "random"), 2, 4)
    assert t.target.tolist() == [1] * 4


def test_curves_under_mask_padding_with_ragged_lengths():
    dev = _dev()
    _, ops, F = _mods()
    model = _tiny_sbm(dev, mask_padding=True)
    lengths = [T_, 20, 9]
    mask = (torch.arange(T_)[None, :] < torch.tensor(lengths)[:, None]).float().to(dev)
    x = _x(dev, seed=6) * mask[:, :, None]
    steps = 3
    f = F.faithfulness_curves(model, x, mask=mask, steps=steps, attributions=("evidence", "random"), fill="mean")
    _check_shapes(f, ("evidence", "random"), steps, B_)
    with torch.no_grad():
        plain = model(x, mask)[0]
        mean = (x.sum(1) / torch.tensor(lengths, device=dev)[:, None])[:, None, :].expand(-1, T_, -1) * mask[:, :, None]
        flat = model(mean.contiguous(), mask)[0]
    for a in f.logit:
        assert torch.equal(f.logit[a][0], plain.gather(1, f.target[:, None]).squeeze(1)), a
        assert torch.equal(f.logit[a][steps], flat.gather(1, f.target[:, None]).squeeze(1)), a       # every own step at its mean
    # only a sample's own steps are ranked and replaced: the padding of every perturbed batch is the padding of x
    k = torch.tensor([[n * C_] for n in lengths], dtype=torch.int32, device=dev)
    ln = torch.tensor(lengths, dtype=torch.int32, device=dev)
    score = torch.rand(B_, T_, C_, device=dev)
    key, idx = ops.rank_threshold(score, k, lengths=ln)
    out = ops.perturb(x, score, key, idx, 0, fill=torch.full((B_, C_), 7.0, device=dev), lengths=ln)
    assert torch.equal(out == 7.0, (mask > 0)[:, :, None].expand(-1, -1, C_))


def test_saliency_raises_what_input_saliency_raises_for_cosine():
    dev = _dev()
    _lib, ops, F = _mods()
    from utils.saliency import input_saliency
    model, x = _tiny_sbm(dev, distance_func="cosine"), _x(dev)
    with pytest.raises(_lib.IgnError) as direct:
        input_saliency(model, x)
    with pytest.raises(_lib.IgnError) as through:
        F.faithfulness_curves(model, x, steps=2, attributions=("saliency",))
    assert str(through.value) == str(direct.value)
    f = F.faithfulness_curves(model, x, steps=2, attributions=("evidence", "random"))                 # these work for every distance
    _check_shapes(f, ("evidence", "random"), 2, B_)
    assert all(m.training is False for m in model.modules())
