"""Attention maps from the fused attention kernels (include/ign_abi.h "Attention map", ign_attn_probs): the map of a call matches a
float64 softmax restatement with the call's dropout mask for every arithmetic, is consistent with the same call's output, is
indexed in 64 bits, leaves the default path bitwise unchanged, and the models / harness run with `output_attention=True`."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import make_cfg
from test_attn_dropout_host import dropout_threshold
from test_gpu_attn_dropout import _Seeds, _dev, _mod, _rel, _set_attn_math, device_mask

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634


def _ref_probs(q, k, scale, bf16=False):
    """float64 softmax(scale Q K^T) (B, H, L, S) on the device.  bf16: the autocast arithmetic's operands, restated as the kernels
    form them -- q * (scale * log2 e) (fp32 product) and k rounded to bf16, the score in base 2."""
    if bf16:
        sc2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
        qb = (q.detach().float() * sc2.to(q.device)).bfloat16().double()
        kb = k.detach().float().bfloat16().double()
        return torch.softmax(torch.einsum("blhe,bshe->bhls", qb, kb) * math.log(2.0), dim=-1)
    return torch.softmax(scale * torch.einsum("blhe,bshe->bhls", q.detach().double(), k.detach().double()), dim=-1)


def _call(ops, amath, q, k, v, scale, p):
    """ops.attention(..., need_weights=True) under the arithmetic `amath` ("bf16" = inside autocast)."""
    if amath == "bf16":
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            return ops.attention(q, k, v, scale, dropout_p=p, need_weights=True)
    return ops.attention(q, k, v, scale, dropout_p=p, need_weights=True)


_SHAPES = [(2, 8, 1000, 1000, 64), (2, 2, 130, 75, 32), (1, 3, 33, 257, 16), (2, 2, 64, 96, 128)]


@pytest.mark.parametrize("B,H,L,S,E", _SHAPES)
@pytest.mark.parametrize("amath", ["f32", "bf16x6", "bf16", "f16x3"])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_map_vs_fp64_and_consistent_with_the_output(B, H, L, S, E, amath, p, monkeypatch):
    dev = _dev()
    _, ops = _mod()
    if E == 128 and amath in ("bf16", "f16x3"):
        pytest.skip("the bf16 and f16x3 arithmetics are instantiated up to E = 64")
    if amath != "bf16":
        _set_attn_math(monkeypatch, ops, amath)
    rec = _Seeds(monkeypatch, ops)
    g = torch.Generator().manual_seed(L + 3 * S + E)
    q = torch.randn(B, L, H, E, generator=g).to(dev)
    k = torch.randn(B, S, H, E, generator=g).to(dev)
    v = torch.randn(B, S, H, E, generator=g).to(dev)
    scale = 1.0 / math.sqrt(E)
    out, attn = _call(ops, amath, q, k, v, scale, p)
    assert attn.shape == (B, H, L, S) and attn.dtype == torch.float32 and attn.is_contiguous()
    ref = _ref_probs(q, k, scale, bf16=(amath == "bf16"))
    if p > 0:
        assert len(rec.seeds) == 1
        Z = device_mask(B, H, L, S, p, rec.seeds[0]).to(dev)
        ref = ref * Z.double() * float(dropout_threshold(p)[1])
        assert torch.equal(attn == 0, ~Z), "exactly the dropped entries are 0"
    else:
        assert not rec.seeds
        assert float((attn.double().sum(-1) - 1.0).abs().max()) < 1e-5, "rows of the p = 0 map sum to 1"
    assert _rel(attn, ref) < (1e-4 if amath == "bf16" else 2e-5), "map vs float64"
    # the map is the one the output was computed with: float64 attn @ v equals the call's out
    av = torch.einsum("bhls,bshd->blhd", attn.double(), v.double())
    assert _rel(out, av) < (3e-2 if amath == "bf16" else 2e-5), "attn @ v vs out"


def test_map_offsets_are_64_bit():
    """B H L S = 264 * 8 * 1024 * 1024 > 2^31 elements (8.9 GB): rows of the last batch and head are the float64 softmax, and a
    strided sample of rows over the whole tensor sums to 1.  With 32-bit offsets the last rows would land elsewhere."""
    dev = _dev()
    _, ops = _mod()
    if ops.GEMM_MATH != "f16x3" or ops.ATTN_MATH != "bf16x6":
        pytest.skip("runs the default (f16x3) arithmetic")
    B, H, L, E = 264, 8, 1024, 64
    assert B * H * L * L > 2 ** 31
    torch.manual_seed(0)
    q, k, v = (torch.randn(B, L, H, E, device=dev) for _ in range(3))
    with torch.no_grad():
        out, attn = ops.attention(q, k, v, 0.125, need_weights=True)
    ref = _ref_probs(q[-1:, :, -1:], k[-1:, :, -1:], 0.125)[0, 0]
    assert _rel(attn[-1, -1], ref) < 2e-5
    rows = attn.view(-1, L)[::4099]
    assert rows.shape[0] > 500
    assert float((rows.double().sum(-1) - 1.0).abs().max()) < 1e-5
    assert float((attn[-1, -1].double().sum(-1) - 1.0).abs().max()) < 1e-5


@pytest.mark.parametrize("amath", ["f32", "bf16x6", "bf16", "f16x3"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_need_weights_leaves_output_gradients_and_rng_bitwise_unchanged(amath, p, monkeypatch):
    dev = _dev()
    _, ops = _mod()
    if amath != "bf16":
        _set_attn_math(monkeypatch, ops, amath)
    g = torch.Generator().manual_seed(17)
    q, k, v = (torch.randn(2, 130, 4, 32, generator=g).to(dev).requires_grad_(True) for _ in range(3))
    go = torch.randn(2, 130, 4, 32, generator=g).to(dev)

    def run(need):
        torch.manual_seed(5)
        if amath == "bf16":
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                res = ops.attention(q, k, v, 0.2, dropout_p=p, need_weights=need)
        else:
            res = ops.attention(q, k, v, 0.2, dropout_p=p, need_weights=need)
        out = res[0] if need else res
        grads = torch.autograd.grad(out, (q, k, v), go)
        return out.detach(), grads, torch.get_rng_state(), (res[1] if need else None)
    o0, g0, s0, _ = run(False)
    o1, g1, s1, attn = run(True)
    assert torch.equal(o0, o1) and all(torch.equal(a, b) for a, b in zip(g0, g1))
    assert torch.equal(s0, s1), "need_weights drew a different number of random numbers"
    assert not attn.requires_grad and attn.grad_fn is None


# ----------------------------------------------------------------------------------------------------------------- models
def _train_step(model_cls, cfg, sd, dev, x, y, igN=False):
    m = model_cls(cfg)
    m.load_state_dict(sd)
    m.to(dev).train()
    torch.manual_seed(42)
    out = m(x, torch.ones(x.shape[0], x.shape[1], device=dev), None, None)
    if igN:
        out, info = out
        loss = F.cross_entropy(out, y) + info.loss.mean() + F.cross_entropy(info.shapelet_preds, y)
    else:
        loss = F.cross_entropy(out, y)
    loss.backward()
    return m, out.detach(), loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def _assert_same_step(a, b):
    _, oa, la, ga = a
    _, ob, lb, gb = b
    assert torch.isfinite(oa).all() and torch.isfinite(la)
    assert torch.equal(oa, ob) and torch.equal(la, lb)
    assert ga.keys() == gb.keys() and all(torch.equal(ga[n], gb[n]) for n in ga), "parameter gradients"


def test_transformer_with_output_attention_trains_bitwise_and_returns_the_maps():
    """Raised NotImplementedError before.  A seeded training step with dropout 0.1 equals the step without the flag bit for bit;
    the encoder returns one (B, H, L, S) map per layer, each the float64 softmax of that layer's q and k (eval mode)."""
    dev = _dev()
    _mod()
    from models.Transformer import Model
    torch.manual_seed(0)
    sd = Model(make_cfg(dropout=0.1)).state_dict()
    x = torch.randn(8, 100, 6, device=dev)
    y = torch.arange(8, device=dev) % 4
    base = _train_step(Model, make_cfg(dropout=0.1), sd, dev, x, y)
    flag = _train_step(Model, make_cfg(dropout=0.1, output_attention=True), sd, dev, x, y)
    _assert_same_step(base, flag)

    m = flag[0].eval()
    cfg = make_cfg()
    seen = []
    hooks = [layer.attention.inner_attention.register_forward_pre_hook(lambda mod, args: seen.append((args[0], args[1])))
             for layer in m.encoder.attn_layers]
    with torch.no_grad():
        _, attns = m.encoder(m.enc_embedding(x, None))
    for hk in hooks:
        hk.remove()
    assert len(attns) == cfg.e_layers == len(seen)
    E = cfg.d_model // cfg.n_heads
    for a, (q, k) in zip(attns, seen):
        assert a.shape == (8, cfg.n_heads, 100, 100)
        assert _rel(a, _ref_probs(q, k, 1.0 / math.sqrt(E))) < 2e-5


@pytest.mark.parametrize("which", ["PatchTST", "InterpGN-Transformer"])
def test_models_with_output_attention_take_the_same_train_step(which):
    dev = _dev()
    _mod()
    if which == "PatchTST":
        from models.PatchTST import Model
        igN, kw = False, {}
    else:
        from models.InterpGN import InterpGN as Model
        igN, kw = True, {"dnn_type": "Transformer"}
    torch.manual_seed(0)
    sd = Model(make_cfg(dropout=0.1, **kw)).state_dict()
    x = torch.randn(8, 100, 6, device=dev)
    y = torch.arange(8, device=dev) % 4
    base = _train_step(Model, make_cfg(dropout=0.1, **kw), sd, dev, x, y, igN)
    flag = _train_step(Model, make_cfg(dropout=0.1, output_attention=True, **kw), sd, dev, x, y, igN)
    _assert_same_step(base, flag)


# ----------------------------------------------------------------------------------------------------------------- harness
def test_experiment_runs_the_transformer_with_output_attention(tmp_path, monkeypatch):
    """`run.py --model DNN --dnn_type Transformer --output_attention` (raised before): one epoch with validation, and test()."""
    _dev()
    _mod()
    import run
    from exp.experiment_classification import Experiment
    monkeypatch.chdir(tmp_path)
    a = run.get_args(["--model", "DNN", "--dnn_type", "Transformer", "--output_attention", "--data", "SYNTH", "--synthetic",
                      "48,6,64,4", "--dataset", "attnmap", "--batch_size", "16", "--amp", "--train_epochs", "1", "--num_workers",
                      "0", "--seed", "0", "--d_model", "32", "--d_ff", "32", "--n_heads", "2", "--e_layers", "2"])
    assert a.output_attention
    run.set_seed(0)
    e = Experiment(a)
    vals, orig = [], e.validation

    def rec():
        r = orig()
        vals.append(r)
        return r
    e.validation = rec
    e.train()
    assert vals and all(math.isfinite(v[0]) for v in vals)
    assert e.test() is not None


def test_hipgraph_with_output_attention_equals_the_eager_run(tmp_path, monkeypatch):
    """InterpGN-Transformer with `--hipgraph --output_attention` (dropout 0): the captured step writes the maps on every replay;
    validation numbers and final weights equal the eager run's, as in test_hipgraph_harness_run_equals_the_eager_run."""
    _dev()
    _mod()
    import run
    from exp.experiment_classification import Experiment
    monkeypatch.chdir(tmp_path)
    outs = {}
    for mode in ("eager", "graph"):
        argv = ["--model", "InterpGN", "--dnn_type", "Transformer", "--output_attention", "--data", "SYNTH", "--synthetic",
                "104,6,100,4", "--dataset", "m" + mode, "--batch_size", "32", "--amp", "--train_epochs", "2", "--num_workers", "0",
                "--seed", "0", "--d_model", "32", "--d_ff", "32", "--n_heads", "2", "--e_layers", "1", "--dropout", "0",
                "--patience", "10"] + (["--hipgraph"] if mode == "graph" else [])
        a = run.get_args(argv)
        run.set_seed(0)
        e = Experiment(a)
        vals, orig = [], e.validation

        def rec(orig=orig, vals=vals):
            r = orig()
            vals.append(r)
            return r
        e.validation = rec
        torch.manual_seed(123)
        e.train()
        outs[mode] = (vals, {k: v.detach().float().cpu().clone() for k, v in e.model.state_dict().items()})
        if mode == "graph":
            assert getattr(e, "_graphed", None) is not None and e.optimizer.capturable      # the graph path really ran
    assert len(outs["eager"][0]) == len(outs["graph"][0]) > 0
    for (la, aa), (lb, ab) in zip(*[o[0] for o in outs.values()]):
        assert abs(la - lb) <= 1e-5 * max(1.0, abs(la)) and aa == ab
    for k, v in outs["eager"][1].items():
        w = outs["graph"][1][k]
        assert float((v - w).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max())), k
