"""Attention dropout inside the fused kernels (include/ign_abi.h "Attention dropout", csrc/ign_dropout.h): the device mask equals
the host restatement bit for bit, every arithmetic matches a float64 restatement built from the dumped mask, p = 0 and eval mode
are unchanged, the mask has the right statistics, a seeded step is reproducible, and the models that raised or silently skipped
the dropout now train with it."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import make_cfg, parity
from test_attn_dropout_host import dropout_threshold, keep_mask

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _mod():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib, ops
    return _lib, ops


def device_mask(B, H, L, S, p, seed):
    """(B, H, L, S) bool keep mask from ign_attn_dropout_mask (the kernels' device function)."""
    _lib, _ = _mod()
    buf = torch.empty(B, H, L, S, dtype=torch.uint8, device="cuda:0")
    _lib.check(_lib.lib().ign_attn_dropout_mask(ctypes.c_void_p(buf.data_ptr()), B, H, L, S, float(p), seed, _lib.stream()),
               "ign_attn_dropout_mask")
    return buf.cpu().bool()


class _Seeds:
    """Records the seed of every dropout call (ops._dropout_seed stays the real one)."""

    def __init__(self, monkeypatch, ops):
        self.seeds = []
        real = ops._dropout_seed

        def rec(p):
            s = real(p)
            self.seeds.append(s)
            return s
        monkeypatch.setattr(ops, "_dropout_seed", rec)


def _set_attn_math(monkeypatch, ops, amath):
    monkeypatch.setattr(ops, "ATTN_MATH", "bf16x6" if amath == "f16x3" else amath)
    monkeypatch.setattr(ops, "GEMM_MATH", "f16x3" if amath == "f16x3" else "bf16x6")


def _ref_dropout_attention(q, k, v, scale, Z, s):
    """(Z o softmax(scale Q K^T)) V s in float64: the reference's dropout(softmax(...)) with the kernels' mask and scale."""
    a = torch.softmax(scale * torch.einsum("blhe,bshe->bhls", q, k), dim=-1) * Z.double() * float(s)
    return torch.einsum("bhls,bshd->blhd", a, v)


# ----------------------------------------------------------------------------------------------------------------- 1. mask
@pytest.mark.parametrize("B,H,L,S,seeds", [(2, 8, 1000, 1000, (0x9E3779B97F4A7C15,)), (3, 8, 100, 100, (0, 1, 2**63 + 12345)),
                                           (2, 3, 33, 257, (7, 0xFFFFFFFFFFFFFFFF, 0xDEADBEEF00000000))])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_device_mask_equals_host_restatement(B, H, L, S, seeds, p):
    _dev()
    for seed in seeds:
        got = device_mask(B, H, L, S, p, seed).numpy()
        want = keep_mask(B, H, L, S, p, seed)
        assert np.array_equal(got, want), f"seed {seed:#x}: {(got != want).sum()} elements differ"


# ----------------------------------------------------------------------------------------------------------------- 2. parity
_SHAPES = [(2, 1000, 1000, 8, 64), (3, 100, 100, 8, 64), (2, 130, 75, 2, 32), (1, 33, 257, 3, 16), (2, 64, 64, 1, 128)]


@pytest.mark.parametrize("B,L,S,H,E", _SHAPES)
@pytest.mark.parametrize("amath", ["f16x3", "f16x3 scaled", "bf16x6", "f32"])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_attention_vs_fp64_reference_with_the_dumped_mask(B, L, S, H, E, amath, p, monkeypatch):
    dev = _dev()
    _, ops = _mod()
    if p == 0.5 and L == 1000 and amath != "f16x3":
        pytest.skip("the full-size shape runs once per arithmetic (p = 0.1) and once at p = 0.5 (f16x3)")
    sq, sk, sv, sg = (1e3, 1e-3, 1e4, 1e-6) if amath.endswith("scaled") else (1.0, 1.0, 1.0, 1.0)
    _set_attn_math(monkeypatch, ops, amath.split()[0])
    rec = _Seeds(monkeypatch, ops)
    g = torch.Generator().manual_seed(L * 7 + E)
    q = (torch.randn(B, L, H, E, generator=g) * sq).to(dev).requires_grad_(True)
    k = (torch.randn(B, S, H, E, generator=g) * sk).to(dev).requires_grad_(True)
    v = (torch.randn(B, S, H, E, generator=g) * sv).to(dev).requires_grad_(True)
    go = torch.randn(B, L, H, E, generator=g) * sg
    scale = 1.0 / math.sqrt(E)
    o = ops.attention(q, k, v, scale, dropout_p=p)
    (o * go.to(dev)).sum().backward()
    assert len(rec.seeds) == 1
    Z = device_mask(B, H, L, S, p, rec.seeds[0])
    _, s = dropout_threshold(p)
    qr, kr, vr = (t.detach().double().cpu().requires_grad_(True) for t in (q, k, v))
    oref = _ref_dropout_attention(qr, kr, vr, scale, Z, s)
    (oref * go.double()).sum().backward()
    assert _rel(o, oref) < 2e-5, "forward"
    for name, a, b in (("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad), ("dv", v.grad, vr.grad)):
        assert _rel(a, b) < 5e-5, name


@pytest.mark.parametrize("B,L,S,H,E", [(2, 200, 200, 4, 64), (2, 130, 75, 2, 32), (1, 33, 257, 3, 16)])
def test_dropout_attention_inside_autocast_is_the_bf16_form(B, L, S, H, E, monkeypatch):
    dev = _dev()
    _, ops = _mod()
    rec = _Seeds(monkeypatch, ops)
    p = 0.1
    g = torch.Generator().manual_seed(L + S + E)
    q, k, v = (torch.randn(B, n, H, E, generator=g).to(dev).requires_grad_(True) for n in (L, S, S))
    go = torch.randn(B, L, H, E, generator=g)
    scale = 1.0 / math.sqrt(E)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        o = ops.attention(q, k, v, scale, dropout_p=p)
    assert o.dtype == torch.float32
    (o * go.to(dev)).sum().backward()
    Z = device_mask(B, H, L, S, p, rec.seeds[0])
    qr, kr, vr = (t.detach().double().cpu().requires_grad_(True) for t in (q, k, v))
    oref = _ref_dropout_attention(qr, kr, vr, scale, Z, dropout_threshold(p)[1])
    (oref * go.double()).sum().backward()
    assert 1e-4 < _rel(o, oref) < 3e-2
    for name, a, b in (("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad), ("dv", v.grad, vr.grad)):
        assert _rel(a, b) < 5e-2, name


@pytest.mark.parametrize("amath", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("B,L,H,E", [(2, 200, 4, 64), (3, 77, 2, 32), (1, 130, 3, 16)])
def test_packed_dropout_attention_and_strided_gradients(B, L, H, E, amath, monkeypatch):
    """ops.attention_packed with dropout: the packed (B, L, 3, H, E) gradient written through the strided backward matches the
    float64 reference, and the unpacked call with the same seed gives the same output and gradients."""
    dev = _dev()
    _, ops = _mod()
    _set_attn_math(monkeypatch, ops, amath)
    rec = _Seeds(monkeypatch, ops)
    p = 0.1
    g = torch.Generator().manual_seed(B + L + H + E)
    qkv = torch.randn(B, L, 3, H, E, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(B, L, H, E, generator=g).to(dev)
    scale = 1.0 / math.sqrt(E)
    torch.manual_seed(11)
    o1 = ops.attention_packed(qkv, scale, dropout_p=p)
    g1, = torch.autograd.grad(o1, qkv, go)
    q, k, v = (qkv[:, :, i].detach().contiguous().requires_grad_(True) for i in range(3))
    torch.manual_seed(11)
    o2 = ops.attention(q, k, v, scale, dropout_p=p)
    gq, gk, gv = torch.autograd.grad(o2, (q, k, v), go)
    assert rec.seeds[0] == rec.seeds[1]
    assert _rel(o1, o2) < 1e-6 and _rel(g1, torch.stack([gq, gk, gv], dim=2)) < 1e-6
    Z = device_mask(B, H, L, L, p, rec.seeds[0])
    qkv_r = qkv.detach().double().cpu().requires_grad_(True)
    oref = _ref_dropout_attention(qkv_r[:, :, 0], qkv_r[:, :, 1], qkv_r[:, :, 2], scale, Z, dropout_threshold(p)[1])
    gref, = torch.autograd.grad(oref, qkv_r, go.double().cpu())
    assert _rel(o1, oref) < 2e-5
    for i, name in enumerate(("dq", "dk", "dv")):
        assert _rel(g1[:, :, i], gref[:, :, i]) < 5e-5, name


# ----------------------------------------------------------------------------------------------------------------- 3. p = 0
@pytest.mark.parametrize("amath", ["f16x3", "bf16x6", "f32"])
def test_p0_is_bitwise_the_dropout_free_path(amath, monkeypatch):
    dev = _dev()
    _, ops = _mod()
    _set_attn_math(monkeypatch, ops, amath)
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(2, 130, 4, 32, generator=g).to(dev).requires_grad_(True) for _ in range(3))
    go = torch.randn(2, 130, 4, 32, generator=g).to(dev)
    state = torch.get_rng_state()
    o0 = ops.attention(q, k, v, 0.2, dropout_p=0.0)
    assert torch.equal(torch.get_rng_state(), state), "p = 0 drew random numbers"
    g0 = torch.autograd.grad(o0, (q, k, v), go)
    o1 = ops.attention(q, k, v, 0.2)
    g1 = torch.autograd.grad(o1, (q, k, v), go)
    assert torch.equal(o0, o1) and all(torch.equal(a, b) for a, b in zip(g0, g1))
    qkv = torch.randn(2, 77, 3, 4, 32, generator=g).to(dev)
    assert torch.equal(ops.attention_packed(qkv, 0.2, dropout_p=0.0), ops.attention_packed(qkv, 0.2))


def test_transformer_in_eval_is_bitwise_the_dropout_free_model():
    dev = _dev()
    _mod()
    from models.Transformer import Model
    torch.manual_seed(0)
    m0 = Model(make_cfg())
    m1 = Model(make_cfg(dropout=0.1))
    m1.load_state_dict(m0.state_dict())
    m0.to(dev).eval()
    m1.to(dev).eval()
    x = torch.randn(8, 100, 6, device=dev)
    mask = torch.ones(8, 100, device=dev)
    with torch.no_grad():
        assert torch.equal(m0(x, mask, None, None), m1(x, mask, None, None))


# ----------------------------------------------------------------------------------------------------------------- 4. statistics
def test_mask_statistics():
    _dev()
    p = 0.1
    thr, _ = dropout_threshold(p)
    q = 1.0 - thr / 65536.0                                         # keep rate actually used
    B, H, L, S = 2, 8, 1000, 1000
    Z = device_mask(B, H, L, S, p, 0x0123456789ABCDEF).numpy()
    n = Z.size
    assert n >= 1.6e7
    frac = Z.mean()
    assert abs(frac - q) < 5 * math.sqrt(q * (1 - q) / n), frac
    # chi^2 of the keep counts per row (B H L rows of S) and per head (B H cells of L S)
    for counts, m in ((Z.sum(axis=3).ravel(), S), (Z.sum(axis=(2, 3)).ravel(), L * S)):
        chi2 = float((((counts - m * q) ** 2) / (m * q * (1 - q))).sum())
        dof = counts.size
        assert abs(chi2 - dof) < 5 * math.sqrt(2 * dof), (chi2, dof)
    zc = Z.astype(np.float64) - q
    var = q * (1 - q)

    def corr(a, b):
        return float((a * b).mean() / var), 5.0 / math.sqrt(a.size)
    for name, (a, b) in {"adjacent keys": (zc[..., :-1], zc[..., 1:]), "adjacent queries": (zc[:, :, :-1], zc[:, :, 1:]),
                         "keys 4 apart": (zc[..., :-4], zc[..., 4:]), "queries 4 apart": (zc[:, :, :-4], zc[:, :, 4:]),
                         "neighbouring heads": (zc[:, :-1], zc[:, 1:]), "batches": (zc[:1], zc[1:])}.items():
        c, lim = corr(a, b)
        assert abs(c) < lim, (name, c, lim)
    # two consecutive calls: different, uncorrelated masks
    _, ops = _mod()
    torch.manual_seed(3)
    s1, s2 = ops._dropout_seed(p), ops._dropout_seed(p)
    Z1, Z2 = device_mask(1, 8, 1000, 1000, p, s1).numpy(), device_mask(1, 8, 1000, 1000, p, s2).numpy()
    assert s1 != s2 and not np.array_equal(Z1, Z2)
    c, lim = corr(Z1.astype(np.float64) - q, Z2.astype(np.float64) - q)
    assert abs(c) < lim, ("consecutive calls", c)


def test_mean_output_over_seeds_converges_to_the_dropout_free_output():
    dev = _dev()
    _, ops = _mod()
    g = torch.Generator().manual_seed(9)
    q, k, v = (torch.randn(1, 64, 2, 16, generator=g).to(dev) for _ in range(3))
    o0 = ops.attention(q, k, v, 0.25).double()
    torch.manual_seed(1)
    outs = torch.stack([ops.attention(q, k, v, 0.25, dropout_p=0.1).double() for _ in range(256)])
    mean, se = outs.mean(0), outs.std(0) / math.sqrt(256)
    z = ((mean - o0).abs() / se.clamp_min(1e-12)).max().item()
    assert z < 5.5, z                                                  # max over 2048 elements of |N(0, 1)|
    assert not torch.equal(outs[0], outs[1])


# ----------------------------------------------------------------------------------------------------------------- 5. determinism
def test_seeded_transformer_train_step_is_bitwise_reproducible():
    dev = _dev()
    _mod()
    from models.Transformer import Model

    def step(seed):
        torch.manual_seed(0)
        m = Model(make_cfg(dropout=0.1)).to(dev).train()
        x = torch.randn(16, 100, 6, device=dev)
        y = torch.arange(16, device=dev) % 4
        torch.manual_seed(seed)
        out = m(x, torch.ones(16, 100, device=dev), None, None)
        F.cross_entropy(out, y).backward()
        return out.detach().clone(), [p.grad.clone() for p in m.parameters() if p.grad is not None]
    o1, g1 = step(42)
    o2, g2 = step(42)
    o3, _ = step(43)
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert not torch.equal(o1, o3)


# ----------------------------------------------------------------------------------------------------------------- 6. models
def _transformer_ref(p, x, mask, n_layers, n_heads, masks, s):
    """float64 restatement of the Transformer baseline (IGN/model/Transformer.py:99-110; the embedding, encoder layers and head
    of oracle/baselines_oracle.py) with dropout(softmax(...)) = Z o softmax(...) s in every attention, the other dropouts 0."""
    from oracle.experts_oracle import _layer_norm, _token_embedding
    h = _token_embedding(p, "enc_embedding", x)
    N, P, D = h.shape
    E = D // n_heads
    for i in range(n_layers):
        lp = f"encoder.attn_layers.{i}"
        q, k, v = ((h @ p[f"{lp}.attention.{n}_projection.weight"].t() + p[f"{lp}.attention.{n}_projection.bias"]).view(N, P, n_heads, E)
                   for n in ("query", "key", "value"))
        o = _ref_dropout_attention(q, k, v, 1.0 / math.sqrt(E), masks[i], s).reshape(N, P, D)
        o = o @ p[lp + ".attention.out_projection.weight"].t() + p[lp + ".attention.out_projection.bias"]
        h = _layer_norm(p, lp + ".norm1", h + o)
        y = F.gelu(h @ p[lp + ".conv1.weight"].squeeze(-1).t() + p[lp + ".conv1.bias"])
        y = y @ p[lp + ".conv2.weight"].squeeze(-1).t() + p[lp + ".conv2.bias"]
        h = _layer_norm(p, lp + ".norm2", h + y)
    h = _layer_norm(p, "encoder.norm", h)
    out = F.gelu(h) * mask[:, :, None].to(h.dtype)
    return out.reshape(N, -1) @ p["projection.weight"].t() + p["projection.bias"]


def test_transformer_with_attention_dropout_trains_and_matches_the_reference(monkeypatch):
    """Transformer baseline (BasicMotions shape) with dropout 0.1 in train mode: raised NotImplementedError before.  Logits and
    every gradient match a float64 restatement fed the kernels' masks (the non-attention dropouts set to 0)."""
    dev = _dev()
    _, ops = _mod()
    from models.Transformer import Model
    rec = _Seeds(monkeypatch, ops)
    cfg = make_cfg(dropout=0.1)
    torch.manual_seed(0)
    m = Model(cfg)
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.Dropout) and not name.endswith("inner_attention.dropout"):
            mod.p = 0.0
    m.to(dev).train()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(8, 100, 6, generator=g)
    mask = torch.ones(8, 100)
    mask[3, 80:] = 0
    y = torch.arange(8) % 4
    out = m(x.to(dev), mask.to(dev), None, None)
    F.cross_entropy(out, y.to(dev)).backward()
    assert len(rec.seeds) == cfg.e_layers
    _, s = dropout_threshold(0.1)
    masks = [device_mask(8, cfg.n_heads, 100, 100, 0.1, sd) for sd in rec.seeds]
    p64 = {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.state_dict().items() if v.is_floating_point()}
    ref = _transformer_ref(p64, x.double(), mask.double(), cfg.e_layers, cfg.n_heads, masks, s)
    F.cross_entropy(ref, y).backward()
    parity("attn_dropout transformer logits", out, ref, tol=1e-4, kind="scale", ref_is="float64 restatement")
    for n, prm in m.named_parameters():
        if prm.grad is None:                                          # the temporal embedding is not evaluated (timeF, no marks)
            assert p64[n].grad is None, n
            continue
        if n.endswith("key_projection.bias"):
            # softmax is invariant to one constant added to every key: an identically zero gradient (both sides rounding noise)
            assert float(prm.grad.abs().max()) <= 1e-7 and float(p64[n].grad.abs().max()) <= 1e-7, n
            continue
        parity(f"attn_dropout transformer d{n}", prm.grad, p64[n].grad, tol=1e-4, kind="scale", floor=1e-6,
               ref_is="float64 restatement")


def test_eegcnn_encoder_layer_applies_self_attn_dropout(monkeypatch):
    """One nn.TransformerEncoderLayer of the EEG-CNN encoder with dropout 0.1 on self_attn only: equal to the no-dropout output
    before (the dropout was skipped), now the float64 restatement with the kernels' mask, gradients included."""
    dev = _dev()
    _, ops = _mod()
    from models.eegcnn import _encoder_layer_forward
    rec = _Seeds(monkeypatch, ops)
    torch.manual_seed(0)
    d, nh = 128, 8
    layer = torch.nn.TransformerEncoderLayer(d, nh, dim_feedforward=256, dropout=0.0, batch_first=True)
    layer.self_attn.dropout = 0.1
    layer.to(dev).train()
    x = torch.randn(4, 40, d, device=dev, requires_grad=True)
    out = _encoder_layer_forward(layer, x, nh)
    go = torch.randn_like(out)
    out.backward(go)
    assert len(rec.seeds) == 1
    Z = device_mask(4, nh, 40, 40, 0.1, rec.seeds[0])
    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in layer.state_dict().items()}
    xr = x.detach().double().cpu().requires_grad_(True)
    B, S, D = xr.shape
    E = D // nh
    qkv = xr @ p["self_attn.in_proj_weight"].t() + p["self_attn.in_proj_bias"]
    q, k, v = (t.reshape(B, S, nh, E) for t in qkv.split(D, dim=-1))
    o = _ref_dropout_attention(q, k, v, 1.0 / math.sqrt(E), Z, dropout_threshold(0.1)[1]).reshape(B, S, D)
    o = o @ p["self_attn.out_proj.weight"].t() + p["self_attn.out_proj.bias"]
    h = F.layer_norm(xr + o, (D,), p["norm1.weight"], p["norm1.bias"], layer.norm1.eps)
    yy = F.relu(h @ p["linear1.weight"].t() + p["linear1.bias"]) @ p["linear2.weight"].t() + p["linear2.bias"]
    ref = F.layer_norm(h + yy, (D,), p["norm2.weight"], p["norm2.bias"], layer.norm2.eps)
    ref.backward(go.double().cpu())
    with torch.no_grad():
        layer.eval()
        no_drop = _encoder_layer_forward(layer, x, nh)
    assert _rel(out, no_drop) > 1e-3, "self_attn dropout had no effect"
    parity("attn_dropout eegcnn layer out", out, ref, tol=1e-4, kind="scale", ref_is="float64 restatement")
    parity("attn_dropout eegcnn layer dx", x.grad, xr.grad, tol=1e-4, kind="scale", ref_is="float64 restatement")
    for n, prm in layer.named_parameters():
        parity(f"attn_dropout eegcnn layer d{n}", prm.grad, p[n].grad, tol=1e-4, kind="scale", floor=1e-6,
               ref_is="float64 restatement")


@pytest.mark.parametrize("which", ["PatchTST", "InterpGN-Transformer"])
def test_models_with_attention_dropout_take_a_finite_train_step(which):
    dev = _dev()
    _mod()
    torch.manual_seed(0)
    if which == "PatchTST":
        from models.PatchTST import Model
        m = Model(make_cfg(dropout=0.1)).to(dev).train()
        out = m(torch.randn(8, 100, 6, device=dev), torch.ones(8, 100, device=dev), None, None)
        loss = F.cross_entropy(out, torch.arange(8, device=dev) % 4)
    else:
        from models.InterpGN import InterpGN
        m = InterpGN(make_cfg(dropout=0.1, dnn_type="Transformer")).to(dev).train()
        out, info = m(torch.randn(8, 100, 6, device=dev), torch.ones(8, 100, device=dev), None, None)
        y = torch.arange(8, device=dev) % 4
        loss = F.cross_entropy(out, y) + info.loss.mean() + F.cross_entropy(info.shapelet_preds, y)
    loss.backward()
    assert torch.isfinite(out).all() and torch.isfinite(loss)
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


def test_graph_capture_with_attention_dropout_is_refused_and_eager_is_chosen():
    dev = _dev()
    _lib, ops = _mod()
    from types import SimpleNamespace
    from exp.experiment_classification import Experiment
    from models.Transformer import Model
    q = torch.randn(2, 64, 2, 16, device=dev)
    ops.attention(q, q, q, 0.25, dropout_p=0.1)                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.IgnError, match="capture"):
        with torch.cuda.graph(graph):
            ops.attention(q, q, q, 0.25, dropout_p=0.1)
    torch.cuda.synchronize()
    assert Experiment._attention_dropout_active(SimpleNamespace(model=Model(make_cfg(dropout=0.1))))
    assert not Experiment._attention_dropout_active(SimpleNamespace(model=Model(make_cfg())))
