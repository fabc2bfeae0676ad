"""GPU parity of the two baselines: the fused fp32-MFMA attention core, the Transformer-encoder model and the EEG-CNN
model, against golden fixtures produced by the reference and against a plain fp32 torch reference of the same op."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, make_cfg, parity, sd_from

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rel(a, b):
    a = a.detach().double().cpu()
    b = torch.as_tensor(np.asarray(b)).double() if not torch.is_tensor(b) else b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _attn_ref(q, k, v, scale):
    """The reference formula (SelfAttention_Family.py:56-75) in float64 on the CPU."""
    q, k, v = (t.detach().double().cpu() for t in (q, k, v))
    s = torch.einsum("blhe,bshe->bhls", q, k)
    return torch.einsum("bhls,bshd->blhd", torch.softmax(scale * s, dim=-1), v)


def _set_attn_math(monkeypatch, ops, amath):
    """"f16x3": two fp16 planes, three products (the default); "bf16x6": three bf16 planes, six products; "f32": fp32 MFMA"""
    monkeypatch.setattr(ops, "ATTN_MATH", "bf16x6" if amath == "f16x3" else amath)
    monkeypatch.setattr(ops, "GEMM_MATH", "f16x3" if amath == "f16x3" else "bf16x6")


@pytest.mark.parametrize("amath", ["f16x3", "bf16x6", "f32"])
def test_attention_core_golden(amath, monkeypatch):
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    _set_attn_math(monkeypatch, ops, amath)
    g = golden("attention_core")
    q, k, v = (_t(g[n], dev).requires_grad_(True) for n in ("q", "k", "v"))
    o = ops.attention(q, k, v, 1.0 / math.sqrt(q.shape[-1]))
    (o * _t(g["go"], dev)).sum().backward()
    for lab, a, b in (("o", o, g["o"]), ("gq", q.grad, g["gq"]), ("gk", k.grad, g["gk"]), ("gv", v.grad, g["gv"])):
        parity(lab, a, b, kind="scale")


@pytest.mark.parametrize("B,L,S,H,E", [(2, 1000, 1000, 8, 64), (3, 100, 100, 8, 64), (2, 130, 75, 2, 32),
                                       (1, 33, 257, 3, 16), (2, 64, 64, 1, 128)])
@pytest.mark.parametrize("amath", ["f16x3", "f16x3 scaled", "bf16x6", "f32"])
def test_attention_vs_fp64_reference(B, L, S, H, E, amath, monkeypatch):
    """"f16x3 scaled": q of magnitude 1e3 against k of 1e-3, v of 1e4 and an output gradient of 1e-6 -- the operand scaling of the
    fp16 kernels must make fp16's exponent range invisible."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    sq, sk, sv, sg = (1e3, 1e-3, 1e4, 1e-6) if amath.endswith("scaled") else (1.0, 1.0, 1.0, 1.0)
    _set_attn_math(monkeypatch, ops, amath.split()[0])
    g = torch.Generator().manual_seed(L * 7 + E)
    q = (torch.randn(B, L, H, E, generator=g) * sq).to(dev).requires_grad_(True)
    k = (torch.randn(B, S, H, E, generator=g) * sk).to(dev).requires_grad_(True)
    v = (torch.randn(B, S, H, E, generator=g) * sv).to(dev).requires_grad_(True)
    go = torch.randn(B, L, H, E, generator=g) * sg
    scale = 1.0 / math.sqrt(E)
    o = ops.attention(q, k, v, scale)
    (o * go.to(dev)).sum().backward()
    qr, kr, vr = (t.detach().double().cpu().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("blhe,bshe->bhls", qr, kr)
    oref = torch.einsum("bhls,bshd->blhd", torch.softmax(scale * s, dim=-1), vr)
    (oref * go.double()).sum().backward()
    assert _rel(o, oref) < 2e-5, "forward"
    for name, a, b in (("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad), ("dv", v.grad, vr.grad)):
        assert _rel(a, b) < 5e-5, name


@pytest.mark.parametrize("amath", ["f16x3", "bf16x6"])
def test_attention_packed_qkv_strides_and_determinism(amath, monkeypatch):
    """q/k/v as strided views of one packed (B,S,3,H,E) projection (the nn.MultiheadAttention in_proj layout)."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    _set_attn_math(monkeypatch, ops, amath)
    torch.manual_seed(3)
    B, S, H, E = 4, 100, 8, 64
    qkv = torch.randn(B, S, 3, H, E, device=dev, requires_grad=True)
    o1 = ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], 0.125)
    g1, = torch.autograd.grad(o1.sum() + (o1 * o1).sum(), qkv, retain_graph=True)
    o2 = ops.attention(qkv[:, :, 0].contiguous(), qkv[:, :, 1].contiguous(), qkv[:, :, 2].contiguous(), 0.125)
    # bf16 planes: layout-independent to the bit.  fp16 planes: the strided views share the packed tensor's bound, the copies
    # have their own -- a different power-of-two scale moves which tiny elements round in fp16's subnormal range
    assert torch.equal(o1, o2) if amath == "bf16x6" else _rel(o1, o2) < 1e-6
    g2, = torch.autograd.grad(o1.sum() + (o1 * o1).sum(), qkv)
    assert torch.equal(g1, g2), "backward not bitwise reproducible"
    oref = _attn_ref(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], 0.125)
    assert _rel(o1, oref) < 2e-5


def test_transformer_baseline_golden():
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from models.Transformer import Model
    g = golden("transformer_bm")
    m = Model(make_cfg())
    assert set(m.state_dict().keys()) == {k[3:] for k in g if k.startswith("sd.")}
    m.load_state_dict(sd_from(g))
    m.to(dev).train()
    x, mask, y = _t(g["x"], dev), _t(g["mask"], dev), _t(g["y"], dev)
    out = m(x, mask, None, None)
    loss = F.cross_entropy(out, y)
    loss.backward()
    parity("out", out, g["out"], kind="elem", f64=g.get("out64"))
    parity("loss", loss, g["loss"], kind="elem")
    gmax = max(float(np.abs(g[k]).max()) for k in g if k.startswith("grad."))
    for n, p in m.named_parameters():
        if "grad." + n not in g:                 # temporal_embedding: constructed but never called on this path
            assert p.grad is None, n
            continue
        if float(np.abs(g["grad." + n]).max()) < 1e-5 * gmax:
            # key_projection.bias has a TRUE gradient of zero (softmax is shift-invariant); both sides hold 1e-9 noise
            assert float(p.grad.abs().max()) < 1e-5 * gmax, f"{n}: not noise-level"
            continue
        parity("grad." + n, p.grad, g["grad." + n], kind="scale", floor=1e-4 * gmax, f64=g.get("grad64." + n))


def test_eegcnn_baseline_golden():
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from models.eegcnn import EEGCNNTransformer
    g = golden("eegcnn_ch")
    m = EEGCNNTransformer(make_cfg(enc_in=122, seq_len=1000, num_class=3, c_out=3, d_model=128))
    sd = sd_from(g)
    missing = set(m.state_dict().keys()) - set(sd)
    assert missing == {"pos_encoder.pe"}, missing           # the sin/cos table is deterministic, not in the fixture
    m.load_state_dict(sd, strict=False)
    m.to(dev).train()
    x, y = _t(g["x"], dev), _t(g["y"], dev)
    out, info = m(x)
    loss = F.cross_entropy(out, y) + info.loss.mean()
    loss.backward()
    feat = m.eegcnn(x)              # same order as the fixture script: two train-mode passes update the BN stats twice
    parity("feat", feat, g["feat"], kind="elem", f64=g.get("feat64"))
    parity("out", out, g["out"], kind="elem", f64=g.get("out64"))
    parity("loss", loss, g["loss"], kind="elem")
    for n, p in m.named_parameters():
        ref = g["grad." + n]
        scale = max(float(np.abs(ref).max()), 1e-7)
        if scale < 1e-5:       # e.g. block1_bn1.bias: a per-channel constant removed again by block1_bn2 -> true grad 0
            # (the fused BatchNorm-2 op returns NO gradient for the constant it cancels: exact zero instead of noise)
            assert p.grad is None or float(p.grad.abs().max()) < 1e-5, f"{n}: not noise-level"
            continue
        parity("grad." + n, p.grad, ref, kind="scale", f64=g.get("grad64." + n))
    for k in (k for k in g if k.startswith("sd_after.")):
        parity(k, m.state_dict()[k[9:]], g[k], kind="elem", f64=g.get("sd_after64." + k[9:]))
    m.eval()
    with torch.no_grad():
        oe, _ = m(x)
    parity("eval_out", oe, g["eval_out"], kind="elem", f64=g.get("eval_out64"))
    with pytest.raises(ValueError):
        m(x, torch.ones(4, 1000, device=dev))                # the reference's mask path cannot run (D9)


@pytest.mark.parametrize("R,T,F1,k1", [(12, 100, 8, 125), (7, 333, 8, 25), (5, 1000, 8, 125), (6, 64, 3, 8), (4, 50, 11, 5)])
def test_conv1_sumsq_vs_torch(R, T, F1, k1):
    """sum (w1 (*) x - mu)^2 and its gradient, against autograd through F.conv1d in float64."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    g = torch.Generator().manual_seed(R * 31 + k1)
    x = (torch.randn(R, T, generator=g) * 1.5 + 0.3).to(dev)
    w = (torch.randn(F1, k1, generator=g) * 0.2).to(dev).requires_grad_(True)
    pl = (k1 - 1) // 2
    xd, wd = x.double().cpu(), w.detach().double().cpu().requires_grad_(True)
    y = F.conv1d(F.pad(xd.unsqueeze(1), (pl, k1 - 1 - pl)), wd.unsqueeze(1))          # (R,F1,T)
    mu = y.mean(dim=(0, 2))
    m2_ref = ((y - mu.view(1, -1, 1)) ** 2).sum(dim=(0, 2))
    cot = torch.randn(F1, generator=g).double()
    (m2_ref * cot).sum().backward()
    m2 = ops.conv1_sumsq(x, w, mu.detach().float().to(dev), pl)
    (m2 * cot.float().to(dev)).sum().backward()
    assert _rel(m2, m2_ref) < 2e-5
    assert _rel(w.grad, wd.grad) < 1e-4        # (the reference grad includes d/dmu = 0 exactly: mu is the batch mean)


# the last ten shapes: at least 32 samples per channel at short rows -- a pass of the cross-correlation kernel then holds many rows
# (round-2 advisor finding: its register prefetch covered fewer rows than a pass, the tail rows multiplied unwritten LDS)
@pytest.mark.parametrize("B,C,T,k", [(3, 64, 500, 25), (2, 64, 1000, 125), (2, 5, 37, 4), (1, 3, 16, 16)] +
                         [(40, 3, T, k) for T in (16, 64, 100, 128, 250) for k in (25, 125)] + [(1100, 2, 64, 25)])
def test_dwconv1d_vs_torch(B, C, T, k):
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    g = torch.Generator().manual_seed(T + k)
    x = torch.randn(B, C, T, generator=g).to(dev).requires_grad_(True)
    w = torch.randn(C, k, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(B, C, T, generator=g)
    pl = (k - 1) // 2
    y = ops.dwconv1d(x, w, pl)
    (y * go.to(dev)).sum().backward()
    xd, wd = x.detach().double().cpu().requires_grad_(True), w.detach().double().cpu().requires_grad_(True)
    yr = F.conv1d(F.pad(xd, (pl, k - 1 - pl)), wd.unsqueeze(1), groups=C)
    (yr * go.double()).sum().backward()
    assert _rel(y, yr) < 1e-5 and _rel(x.grad, xd.grad) < 1e-5 and _rel(w.grad, wd.grad) < 2e-5


def _eegcnn_reference_ops(m, x):
    """IGN/model/eegcnn.py:85-108 layer by layer on the module's own nn layers (torch / library kernels): the op-by-op evaluation
    the HIP restructuring of models/eegcnn.py is checked against."""
    x = x.unsqueeze(1)                                           # (B,1,C,T)
    x = m.block1_bn1(m.block1_conv1(x))
    x = m.block1_bn2(m.block1_depthwise(x))
    x = m.block1_drop(m.block1_pool(m.block1_elu(x)))
    x = m.block2_conv2(m.block2_conv1(x))
    x = m.block2_drop(m.block2_pool(m.block2_elu(m.block2_bn(x))))
    return x.squeeze(2)                                          # (B,F2,T')


def test_eegcnn_block_matches_reference_ops_in_eval_and_train():
    """The algebraic restructuring of block 1/2 against the layer-by-layer evaluation of the same module (torch ops),
    including BatchNorm running statistics."""
    dev = _dev()
    import copy
    import speech_imagery_eeg_amd  # noqa
    from models.eegcnn import EEGcnn
    torch.manual_seed(0)
    m = EEGcnn(Chans=20, kernLength1=31, kernLength2=8, F1=4, D=3, F2=12, P1=2, P2=5, dropoutRate=0.0).to(dev)
    with torch.no_grad():
        for bn in (m.block1_bn1, m.block1_bn2, m.block2_bn):
            bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.5, 0.5)
    ref = copy.deepcopy(m)
    x = torch.randn(6, 20, 200, device=dev) * 2 + 0.5
    for mode in (True, False):
        m.train(mode); ref.train(mode)
        a = m(x)
        b = _eegcnn_reference_ops(ref, x)
        parity(f"out train={mode}", a, b, kind="scale", ref_is="same module, layer-by-layer torch ops (fp32, GPU)")
        if mode:
            ga = torch.autograd.grad(a.square().sum(), [p for p in m.parameters()], allow_unused=True)
            gb = torch.autograd.grad(b.square().sum(), [p for p in ref.parameters()])
            for (n, _), u, v in zip(m.named_parameters(), ga, gb):
                sc = float(v.abs().max())
                if sc < 1e-4 * float(max(t.abs().max() for t in gb)):
                    continue                      # zero-gradient parameters (bias removed by the next BatchNorm)
                assert u is not None, n
                parity("grad." + n, u, v, kind="scale", ref_is="same module, layer-by-layer torch ops (fp32, GPU)")
            for k in m.state_dict():
                parity("sd." + k, m.state_dict()[k].float(), ref.state_dict()[k].float(), kind="scale",
                       ref_is="same module, layer-by-layer torch ops (fp32, GPU)")


@pytest.mark.parametrize("T,k1", [(64, 25), (128, 125), (250, 125), (100, 25)])
def test_eegcnn_train_step_at_short_rows_with_many_samples(T, k1):
    """An EEGcnn training step (forward, backward, BatchNorm statistics) at short rows and 48 samples -- every pass of the
    cross-correlation kernel is full -- against the layer-by-layer evaluation of the same module."""
    dev = _dev()
    import copy
    import speech_imagery_eeg_amd  # noqa
    from models.eegcnn import EEGcnn
    torch.manual_seed(T + k1)
    m = EEGcnn(Chans=9, kernLength1=k1, kernLength2=25, F1=4, D=2, F2=8, P1=2, P2=4, dropoutRate=0.0).to(dev)
    ref = copy.deepcopy(m).double().cpu()          # float64 on the host: the fp32 library convolutions are themselves 3e-4 off here
    x = torch.randn(48, 9, T, device=dev) * 1.5 + 0.2
    m.train(); ref.train()
    a, b = m(x), _eegcnn_reference_ops(ref, x.double().cpu())
    assert torch.isfinite(a).all()
    parity(f"short rows T={T} k={k1}: out", a, b, kind="scale", ref_is="same module, layer-by-layer torch ops (float64, CPU)")
    ga = torch.autograd.grad(a.square().sum(), list(m.parameters()), allow_unused=True)
    gb = torch.autograd.grad(b.square().sum(), list(ref.parameters()))
    top = float(max(t.abs().max() for t in gb))
    for (n, _), u, v in zip(m.named_parameters(), ga, gb):
        if float(v.abs().max()) < 1e-4 * top:
            continue                              # zero-gradient parameters (bias removed by the next BatchNorm)
        assert u is not None and torch.isfinite(u).all(), n
        parity(f"short rows T={T} k={k1}: grad." + n, u, v, kind="scale", ref_is="same module, layer-by-layer torch ops (float64, CPU)")


# second list: row-count edges of the 128 x 128-tile k = 1 weight-gradient kernel (clconv_wgrad_x6_k1_kernel) on both split arithmetics
# -- one row; less than a 16-row unit; a ragged second unit over two ci / co tiles; 33 units = 2 splits with 11 live rows in the last
# unit; 257 units = 9 splits, i.e. a second round over the 8 XCDs whose surplus workgroups return early
_LINEAR_CASES = [pytest.param(shape, Co, bias, *arith, id="-".join(map(str, arith)) + f"-shape{i}-{Co}-{bias}")     # (ids as before the
                 for i, (shape, Co, bias) in enumerate([((256, 100, 512), 256, True), ((3, 77, 64), 512, True),    # second list existed)
                                                        ((5, 130), 12, False), ((2, 1000, 512), 2048, True)])
                 for arith in [("bf16x6", "bf16x6", 1.0), ("f32", "bf16x6", 1.0), ("bf16x6", "f16x3", 1.0), ("bf16x6", "f16x3", 1e-6),
                               ("bf16x6", "f16x3", 1e5)]] + \
                [pytest.param((M, Ci), Co, True, *arith, id="-".join(map(str, arith)) + f"-rows{M}x{Ci}-{Co}-True")
                 for M, Ci, Co in [(1, 4, 4), (15, 8, 12), (17, 132, 132), (523, 128, 64), (4100, 64, 64)]
                 for arith in [("bf16x6", "bf16x6", 1.0), ("bf16x6", "f16x3", 1.0)]]


@pytest.mark.parametrize("shape,Co,bias,wgrad,gmath,scale", _LINEAR_CASES)
def test_linear_on_own_gemm_kernels(shape, Co, bias, wgrad, gmath, scale, monkeypatch):
    """ops.linear (forward / input gradient / weight gradient on the split kernels: six-product bf16 or three-product fp16 with
    power-of-two operand scaling; weight gradient alternatively on the fp32-MFMA TN kernel) against float64 torch.  `scale`:
    activations of magnitude 1e5 and output gradients of 1e-6 (and the other way round) -- fp16's exponent range must not show."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    monkeypatch.setattr(ops, "LINEAR_WGRAD", wgrad)
    monkeypatch.setattr(ops, "GEMM_MATH", gmath)
    g = torch.Generator().manual_seed(sum(shape) + Co)
    Ci = shape[-1]
    x = torch.randn(*shape, generator=g) * scale
    w = torch.randn(Co, Ci, generator=g) / Ci ** 0.5
    b = torch.randn(Co, generator=g) * scale if bias else None
    gy = torch.randn(*shape[:-1], Co, generator=g) / scale
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    bd = b.double().requires_grad_(True) if bias else None
    (F.linear(xd, wd, bd) * gy.double()).sum().backward()
    xg, wg = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    bg = b.to(dev).requires_grad_(True) if bias else None
    y = ops.linear(xg, wg, bg)
    (y * gy.to(dev)).sum().backward()
    assert _rel(y, F.linear(xd, wd, bd)) < 3e-6
    assert _rel(xg.grad, xd.grad) < 3e-6 and _rel(wg.grad, wd.grad) < 1e-5
    if bias:
        assert _rel(bg.grad, bd.grad) < 1e-5


# ------------------------------------------------------------------------------------------- remaining deep experts
@pytest.mark.parametrize("B,Tin,Ci,Co,k,bias", [(3, 40, 6, 64, 3, False), (2, 130, 12, 64, 4, True), (4, 27, 64, 128, 3, False),
                                                (2, 300, 122, 512, 3, False), (1, 17, 5, 8, 7, True), (2, 64, 128, 128, 1, True),
                                                (3, 33, 7, 12, 11, False)])
@pytest.mark.parametrize("gmath", ["f16x3", "bf16x6"])
def test_conv1d_cl_against_float64(B, Tin, Ci, Co, k, bias, gmath, monkeypatch):
    """ops.conv1d_cl (valid, stride 1, channels-last) forward / input gradient / weight gradient against float64 torch, on the
    three-product fp16 kernels (default) and the six-product bf16 kernels."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    monkeypatch.setattr(ops, "GEMM_MATH", gmath)
    g = torch.Generator().manual_seed(B * 1000 + Tin + Ci + Co + k)
    x = torch.randn(B, Tin, Ci, generator=g)
    w = torch.randn(Co, Ci, k, generator=g) / (Ci * k) ** 0.5
    b = torch.randn(Co, generator=g) if bias else None
    gy = torch.randn(B, Tin - k + 1, Co, generator=g)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    bd = b.double().requires_grad_(True) if bias else None
    yd = F.conv1d(xd.permute(0, 2, 1), wd, bd).permute(0, 2, 1)
    (yd * gy.double()).sum().backward()
    xg, wg = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    bg = b.to(dev).requires_grad_(True) if bias else None
    y = ops.conv1d_cl(xg, wg, bg)
    (y * gy.to(dev)).sum().backward()
    assert _rel(y, yd) < 3e-6
    assert _rel(xg.grad, xd.grad) < 3e-6 and _rel(wg.grad, wd.grad) < 1e-5
    if bias:
        assert _rel(bg.grad, bd.grad) < 1e-5


def _check_expert_golden(m, g, out, loss):
    """Logits / loss element-wise at 1e-4; every gradient at 1e-4 of its scale, the scale floored at 1e-4 of the largest
    gradient in the model (tensors whose true gradient is ~0 -- a bias in front of BatchNorm -- hold rounding noise)."""
    parity("out", out, g["out"], kind="elem", f64=g.get("out64"))
    parity("loss", loss, g["loss"], kind="elem")
    gmax = max(float(np.abs(g[k]).max()) for k in g if k.startswith("grad."))
    for n, p in m.named_parameters():
        if "grad." + n not in g:                 # temporal_embedding: constructed, never called on this path
            assert p.grad is None, n
            continue
        if float(np.abs(g["grad." + n]).max()) < 1e-5 * gmax:        # true-zero gradient: rounding noise on both sides
            assert float(p.grad.abs().max()) < 1e-5 * gmax, f"{n}: not noise-level"
            continue
        parity("grad." + n, p.grad, g["grad." + n], kind="scale", floor=1e-4 * gmax, f64=g.get("grad64." + n))


@pytest.mark.parametrize("tag,C,T,N", [("bm", 6, 100, 4), ("odd", 3, 61, 2)])
def test_resnet_expert_golden(tag, C, T, N):
    """ResNet deep expert on the channels-last implicit-GEMM kernels against the reference's outputs (tests/golden/resnet_*.npz):
    logits, loss, every parameter gradient, BatchNorm running statistics after one training forward, eval-mode logits."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from models.ResNet import Model
    g = golden("resnet_" + tag)
    m = Model(make_cfg(enc_in=C, seq_len=T, num_class=N))
    assert set(m.state_dict().keys()) == {k[3:] for k in g if k.startswith("sd.")}
    m.load_state_dict(sd_from(g))
    m.to(dev).train()
    x, y = _t(g["x"], dev), _t(g["y"], dev)
    out = m(x)
    loss = F.cross_entropy(out, y)
    loss.backward()
    _check_expert_golden(m, g, out, loss)
    sd = m.state_dict()
    for k in g:
        if k.startswith("sd_after."):
            parity(k, sd[k[9:]], g[k], kind="elem")
    m.eval()
    with torch.no_grad():
        parity("eval_out", m(x), g["eval_out"], kind="elem")


def test_patchtst_expert_golden():
    """PatchTST deep expert (patching, the shared encoder on ign_attn_* / ops.linear, streaming class head) against the
    reference's outputs (tests/golden/patchtst_bm.npz)."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from models.PatchTST import Model
    g = golden("patchtst_bm")
    m = Model(make_cfg())
    want = {k[3:] for k in g if k.startswith("sd.")}
    assert {k for k in m.state_dict() if not k.endswith("position_embedding.pe")} == want
    m.load_state_dict(sd_from(g), strict=False)
    m.to(dev).train()
    x, y = _t(g["x"], dev), _t(g["y"], dev)
    out = m(x, None, None, None)
    loss = F.cross_entropy(out, y)
    loss.backward()
    _check_expert_golden(m, g, out, loss)


def test_ign_with_resnet_expert_runs_and_matches_parts():
    """InterpGN with dnn_type='ResNet': the mixture is the gate applied to the two experts' own outputs."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from models.InterpGN import InterpGN, gini_gate
    torch.manual_seed(0)
    m = InterpGN(make_cfg(dnn_type="ResNet")).to(dev).train()
    x = torch.randn(8, 100, 6, device=dev)
    out, info = m(x, torch.ones(8, 100, device=dev), None, None)
    ref, eta = gini_gate(info.shapelet_preds, info.dnn_preds)
    assert _rel(out, ref) < 1e-5 and _rel(info.eta, eta) < 1e-5
    out.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.deep_model.parameters())


def test_timesnet_expert_golden():
    """TimesNet deep expert (fused-inception 2-D convolutions on the 1-D implicit-GEMM kernels, rocFFT period detection)
    against the reference's outputs (tests/golden/timesnet_t96.npz); the periods it folds by must be the reference's."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from models import TimesNet as TN
    g = golden("timesnet_t96")
    m = TN.Model(make_cfg(seq_len=96, d_model=16, d_ff=16, top_k=3, num_kernels=6))
    want = {k[3:] for k in g if k.startswith("sd.")}
    assert {k for k in m.state_dict() if not k.endswith("position_embedding.pe")} == want
    m.load_state_dict(sd_from(g), strict=False)
    m.to(dev).train()
    x, mask, y = _t(g["x"], dev), _t(g["mask"], dev), _t(g["y"], dev)
    with torch.no_grad():
        h = m.enc_embedding(x, None)
        for i, blk in enumerate(m.model):
            assert list(TN.FFT_for_Period(h, 3)[0]) == list(g["periods"][i])
            h = m.layer_norm(blk(h))
    out = m(x, mask, None, None)
    loss = F.cross_entropy(out, y)
    loss.backward()
    _check_expert_golden(m, g, out, loss)


def test_inception_block_fused_equals_separate_convs():
    """The single (2n-1)x(2n-1) convolution on the 1-D kernels equals the mean of the n same-padded Conv2d's (float64)."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from models.TimesNet import Inception_Block_V1
    torch.manual_seed(3)
    blk = Inception_Block_V1(8, 12, num_kernels=4)
    for conv in blk.kernels:
        nn_b = torch.randn_like(conv.bias)
        conv.bias.data.copy_(nn_b)
    x = torch.randn(3, 5, 7, 8)                                              # (B, H, W, C)
    ref = blk.double()(x.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    y = blk.float().to(dev).forward_cl(x.to(dev))
    assert _rel(y, ref) < 3e-6


@pytest.mark.parametrize("name,kw", [("ResNet", {}), ("PatchTST", {}), ("Transformer", {}),
                                     ("TimesNet", dict(seq_len=96, d_model=16, d_ff=16, top_k=3, num_kernels=6))])
def test_deep_experts_inside_autocast_use_the_bf16_kernels(name, kw, monkeypatch):
    """The reference's default mode (bf16 autocast): the deep experts stay on the hand-written kernels, in their single-product
    bf16 form -- logits within bf16 distance of the fp32-accurate run but not equal to it, finite gradients everywhere."""
    dev = _dev()
    import importlib
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import _lib
    L = _lib.lib()
    calls = {"bf16": 0}
    real = L.ign_clconv_fwd_bf16

    class Spy:
        def __getattr__(self, n):
            if n == "ign_clconv_fwd_bf16":
                def f(*a):
                    calls["bf16"] += 1
                    return real(*a)
                return f
            return getattr(L, n)

    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    cfg = make_cfg(**kw)
    torch.manual_seed(0)
    m = importlib.import_module("models." + name).Model(cfg).to(dev).train()
    T = cfg.seq_len
    g = torch.Generator().manual_seed(9)
    t = torch.arange(T, dtype=torch.float32)[None, :, None]
    x = (torch.sin(2 * math.pi * t / 24) * 2 + torch.sin(2 * math.pi * t / 8) + 0.2 * torch.randn(4, T, 6, generator=g)).to(dev)
    mask = torch.ones(4, T, device=dev)
    ref = m(x, mask, None, None)
    assert calls["bf16"] == 0
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        out = m(x, mask, None, None)
    assert calls["bf16"] > 0
    out.float().sum().backward()
    d = _rel(out.float(), ref.float())
    assert 1e-6 < d < 8e-2, d
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


@pytest.mark.parametrize("B,L,S,H,E", [(2, 200, 200, 4, 64), (2, 130, 75, 2, 32), (1, 33, 257, 3, 16)])
def test_attention_inside_autocast_is_the_bf16_single_product_form(B, L, S, H, E):
    """Inside torch.autocast(bfloat16) the attention core rounds Q, K, V, P (and dO, dS) to bf16 and issues one product per MFMA
    step: bf16-level distance from the float64 reference (forward and all three gradients), and not the fp32-accurate result."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    g = torch.Generator().manual_seed(L + S + E)
    q = torch.randn(B, L, H, E, generator=g).to(dev).requires_grad_(True)
    k = torch.randn(B, S, H, E, generator=g).to(dev).requires_grad_(True)
    v = torch.randn(B, S, H, E, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(B, L, H, E, generator=g)
    scale = 1.0 / math.sqrt(E)
    exact = ops.attention(q, k, v, scale).detach()
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        o = ops.attention(q, k, v, scale)
    assert o.dtype == torch.float32
    (o * go.to(dev)).sum().backward()
    qr, kr, vr = (t.detach().double().cpu().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("blhe,bshe->bhls", qr, kr)
    oref = torch.einsum("bhls,bshd->blhd", torch.softmax(scale * s, dim=-1), vr)
    (oref * go.double()).sum().backward()
    assert 1e-4 < _rel(o, oref) < 3e-2 and _rel(exact, oref) < 2e-5
    for name, a, b in (("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad), ("dv", v.grad, vr.grad)):
        assert _rel(a, b) < 5e-2, name


def test_eegcnn_inside_autocast_stays_on_the_hand_written_kernels(monkeypatch):
    """EEG-CNN in the reference's default bf16 mode: the convolution block keeps its fp32 HIP kernels (autocast disabled inside),
    the encoder uses the bf16 single-product GEMM / attention kernels; logits within bf16 distance of the fp32 run."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import _lib
    from models.eegcnn import EEGCNNTransformer
    L = _lib.lib()
    calls = {"bf16": 0, "dw": 0}
    real = {n: getattr(L, n) for n in ("ign_clconv_fwd_bf16", "ign_dwconv1d_fwd")}

    class Spy:
        def __getattr__(self, n):
            if n in real:
                def f(*a, _n=n):
                    calls["bf16" if "bf16" in _n else "dw"] += 1
                    return real[_n](*a)
                return f
            return getattr(L, n)

    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    cfg = make_cfg(enc_in=122, seq_len=1000, num_class=3, c_out=3, d_model=128)
    torch.manual_seed(0)
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        m = EEGCNNTransformer(cfg).to(dev).train()
        x = torch.randn(4, 122, 1000, device=dev)
        ref, _ = m(x)
        assert calls["bf16"] == 0 and calls["dw"] > 0
        calls["dw"] = 0
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            out, _ = m(x)
    assert calls["bf16"] > 0 and calls["dw"] > 0
    out.float().sum().backward()
    d = _rel(out.float(), ref.float())
    assert 1e-6 < d < 8e-2, d
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


@pytest.mark.parametrize("B,L,H,E", [(2, 200, 4, 64), (3, 77, 2, 32), (1, 130, 3, 16)])
def test_packed_attention_equals_unpacked(B, L, H, E):
    """ops.attention_packed on a packed (B, L, 3, H, E) projection: same output as the unpacked call, and the packed gradient
    equals the three separate gradients stacked (written through ign_attn_bwd_x6_strided, no gather)."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    g = torch.Generator().manual_seed(B + L + H + E)
    qkv = torch.randn(B, L, 3, H, E, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(B, L, H, E, generator=g).to(dev)
    scale = 1.0 / math.sqrt(E)
    o1 = ops.attention_packed(qkv, scale)
    g1, = torch.autograd.grad(o1, qkv, go)
    q, k, v = (qkv[:, :, i].detach().contiguous().requires_grad_(True) for i in range(3))
    o2 = ops.attention(q, k, v, scale)
    gq, gk, gv = torch.autograd.grad(o2, (q, k, v), go)
    assert torch.equal(o1, o2)
    assert torch.equal(g1, torch.stack([gq, gk, gv], dim=2))


@pytest.mark.parametrize("R,T,k,pl", [(7, 200, 125, 62), (33, 1000, 125, 62), (5, 64, 25, 12), (3, 130, 8, 0), (2, 129, 128, 127)] +
                         [(70, T, k, (k - 1) // 2) for T in (16, 64, 100, 128, 250) for k in (25, 125) if T >= k // 2])   # rows shorter than the padding: not a model shape
def test_window_gram_matrix_equals_brute_force(R, T, k, pl):
    """EEGcnn._window_gram (lag sums from ign_autocorr_fwd + edge terms) against the brute-force Gram matrix of all padded windows
    in float64, and the quadratic form against sum_t (w (*) x)^2 of the convolution itself."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from models.eegcnn import EEGcnn
    g = torch.Generator().manual_seed(R + T + k)
    x = torch.randn(R, T, generator=g)
    G = EEGcnn._window_gram(x.to(dev), k, pl).cpu()
    xp = F.pad(x.double(), (pl, k - 1 - pl))
    W = xp.unfold(1, k, 1)[:, :T]
    Gref = torch.einsum('rtj,rtk->jk', W, W)
    assert float((G - Gref).abs().max() / Gref.abs().max()) < 2e-6
    w = torch.randn(4, k, generator=g).double()
    y = F.conv1d(xp.unsqueeze(1), w.unsqueeze(1))                                   # (R, 4, T)
    assert _rel(torch.einsum('fj,jk,fk->f', w, G, w), y.square().sum(dim=(0, 2))) < 2e-6


@pytest.mark.parametrize("R,T,k,pl", [(7, 200, 125, 62), (33, 1000, 125, 62), (5, 64, 25, 12), (3, 130, 8, 0), (300, 129, 124, 123),
                                      (2, 40, 2, 1), (700, 125, 125, 0)])
def test_bn1_data_statistics_equal_brute_force(R, T, k, pl):
    """ops.bn1_data_stats (lag sums, edge terms and column sums from two kernels, assembled by ign_bn1_gram) against the
    brute-force Gram matrix and per-tap sums of all zero-padded windows in float64."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    g = torch.Generator().manual_seed(R + T + k)
    x = torch.randn(R, T, generator=g) + 0.3
    G, S = ops.bn1_data_stats(x.to(dev), k, pl)
    xp = F.pad(x.double(), (pl, k - 1 - pl))
    W = xp.unfold(1, k, 1)[:, :T]
    Gref = torch.einsum('rtj,rtk->jk', W, W)
    Sref = W.sum(dim=(0, 1))
    assert float((G.cpu() - Gref).abs().max() / Gref.abs().max()) < 2e-6
    assert float((S.cpu() - Sref).abs().max() / Sref.abs().max()) < 2e-6
    assert torch.equal(G, G.t())


@pytest.mark.parametrize("F1,k,D,track", [(8, 125, 8, True), (3, 25, 2, False), (16, 7, 16, True)])
def test_bn1_fold_against_the_float64_composition(F1, k, D, track):
    """ops.bn1_fold (ign_bn1_fold_fwd / _bwd): BatchNorm-1 with batch statistics as a closed form in the filter -- outputs, the four
    parameter gradients and the running-statistics update against the same algebra written with float64 torch ops and autograd."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    g = torch.Generator().manual_seed(F1 * k + D)
    R, T, pl = 40, 300, (k - 1) // 2
    x = torch.randn(R, T, generator=g) * 2 + 0.7
    G, S = ops.bn1_data_stats(x.to(dev), k, pl)
    n, eps, mom = float(R * T), 1e-5, 0.1
    w1 = (torch.randn(F1, k, generator=g) / k ** 0.5)
    gamma, beta = torch.rand(F1, generator=g) + 0.5, torch.randn(F1, generator=g) * 0.2
    rs = torch.randn(F1 * D, generator=g)
    ga, gc = torch.randn(F1 * D, generator=g), torch.randn(F1 * D, generator=g)
    # reference algebra, float64
    p = [t.double().to(dev).requires_grad_(True) for t in (w1, gamma, beta, rs)]
    mu = p[0] @ S / n
    var = torch.einsum('fj,jk,fk->f', p[0], G, p[0]) / n - mu.square()
    a = p[1] * torch.rsqrt(var + eps)
    b = p[2] - a * mu
    alpha_r, cshift_r = a.repeat_interleave(D), b.repeat_interleave(D) * p[3]
    (alpha_r * ga.double().to(dev) + cshift_r * gc.double().to(dev)).sum().backward()
    q = [t.to(dev).requires_grad_(True) for t in (w1, gamma, beta, rs)]
    rm, rv = torch.full((F1,), 0.25, device=dev), torch.full((F1,), 1.5, device=dev)
    alpha, cshift = ops.bn1_fold(*q, G, S, n, eps, mom if track else 0.0, rm if track else None, rv if track else None, D)
    (alpha * ga.to(dev) + cshift * gc.to(dev)).sum().backward()
    assert _rel(alpha, alpha_r) < 2e-6 and _rel(cshift, cshift_r) < 2e-6
    for name, u, v in zip(("w1", "gamma", "beta", "rs"), q, p):
        assert _rel(u.grad, v.grad) < 1e-5, name
    if track:
        assert _rel(rm, 0.9 * 0.25 + 0.1 * mu.detach()) < 2e-6
        assert _rel(rv, 0.9 * 1.5 + 0.1 * var.detach() * (n / (n - 1))) < 2e-6
    else:
        assert float(rm[0]) == 0.25 and float(rv[0]) == 1.5


@pytest.mark.parametrize("shape", [(1000, 64), (7, 33, 16), (3, 100, 512), (2, 5, 2048), (130, 12), (4, 9, 200), (1, 1, 128)])
@pytest.mark.parametrize("bias", [True, False])
def test_layer_norm_against_float64(shape, bias, monkeypatch):
    """ops.layer_norm (ign_layernorm_fwd / _bwd) against float64 torch: output, input gradient, d(gamma), d(beta); bitwise
    reproducible across calls."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    monkeypatch.setattr(ops, "LAYERNORM_MIN_ROWS", 0)          # exercise the kernels at every size
    D = shape[-1]
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g) * 3 + 1.5
    gy = torch.randn(*shape, generator=g)
    ln = torch.nn.LayerNorm(D, bias=bias)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        if bias:
            ln.bias.normal_(0, 0.3)
    ref = torch.nn.LayerNorm(D, bias=bias).double()
    ref.load_state_dict({k: v.double() for k, v in ln.state_dict().items()})
    xd = x.double().requires_grad_(True)
    (ref(xd) * gy.double()).sum().backward()
    lg = ln.to(dev)
    xg = x.to(dev).requires_grad_(True)
    y = ops.layer_norm(xg, lg)
    (y * gy.to(dev)).sum().backward()
    assert _rel(y, ref(xd)) < 2e-6
    assert _rel(xg.grad, xd.grad) < 5e-6
    assert _rel(lg.weight.grad, ref.weight.grad) < 1e-5
    if bias:
        assert _rel(lg.bias.grad, ref.bias.grad) < 1e-5
    g1 = (xg.grad.clone(), lg.weight.grad.clone())
    xg.grad = None; lg.weight.grad = None
    (ops.layer_norm(xg, lg) * gy.to(dev)).sum().backward()
    assert torch.equal(g1[0], xg.grad) and torch.equal(g1[1], lg.weight.grad)


@pytest.mark.parametrize("shape", [(1000, 64), (3, 100, 512), (2, 5, 2048), (130, 12), (1, 1, 128)])
def test_layer_norm_with_the_residual_add_in_the_same_pass(shape, monkeypatch):
    """ops.layer_norm(x, norm, residual=r) (ign_layernorm_res_fwd) == LayerNorm(x + r): output and all four gradients against
    float64 torch, and bitwise against the two-launch route on the same kernels (torch add, then ign_layernorm_fwd)."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    monkeypatch.setattr(ops, "LAYERNORM_MIN_ROWS", 0)
    D = shape[-1]
    g = torch.Generator().manual_seed(sum(shape) + 1)
    x, r, gy = (torch.randn(*shape, generator=g) * 2 + 0.5, torch.randn(*shape, generator=g), torch.randn(*shape, generator=g))
    ln = torch.nn.LayerNorm(D)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.normal_(0, 0.3)
    ref = torch.nn.LayerNorm(D).double()
    ref.load_state_dict({k: v.double() for k, v in ln.state_dict().items()})
    xd, rd = x.double().requires_grad_(True), r.double().requires_grad_(True)
    yd = ref(xd + rd)
    (yd * gy.double()).sum().backward()
    lg = ln.to(dev)
    res = {}
    for fused in (True, False):
        lg.zero_grad(set_to_none=True)
        xg, rg = x.to(dev).requires_grad_(True), r.to(dev).requires_grad_(True)
        y = ops.layer_norm(xg, lg, residual=rg) if fused else ops.layer_norm(xg + rg, lg)
        (y * gy.to(dev)).sum().backward()
        res[fused] = (y.detach(), xg.grad, rg.grad, lg.weight.grad.clone(), lg.bias.grad.clone())
    y, gx, gr, gw, gb = res[True]
    assert _rel(y, yd) < 2e-6 and _rel(gx, xd.grad) < 5e-6 and _rel(gr, rd.grad) < 5e-6
    assert _rel(gw, ref.weight.grad) < 1e-5 and _rel(gb, ref.bias.grad) < 1e-5
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
    assert gx.data_ptr() != gr.data_ptr() or not (xg.is_leaf and rg.is_leaf)      # two leaves never share one gradient buffer


# ------------------------------------------------------------------ size-independent properties at the benchmark shape (B=256, L=1000)
def test_attention_x6_full_size_batch_independence_and_linearity():
    """B=256, H=8, L=S=1000, E=64 (the Transformer baseline's attention): every sample's output / gradients equal those of a
    2-sample call holding the same samples (bitwise: no cross-sample coupling, no launch-shape dependence), the output is linear
    in V, and permuting the keys leaves it unchanged up to rounding."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    B, L, H, E = 256, 1000, 8, 64
    g = torch.Generator(device="cpu").manual_seed(7)
    q = torch.randn(B, L, H, E, generator=g).to(dev).requires_grad_(True)
    k = torch.randn(B, L, H, E, generator=g).to(dev).requires_grad_(True)
    v = torch.randn(B, L, H, E, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(B, L, H, E, generator=g).to(dev)
    o = ops.attention(q, k, v, 0.125)
    gq, gk, gv = torch.autograd.grad(o, (q, k, v), go)
    idx = [3, 250]
    qs, ks, vs = (t[idx].detach().clone().requires_grad_(True) for t in (q, k, v))
    os_ = ops.attention(qs, ks, vs, 0.125)
    gqs, gks, gvs = torch.autograd.grad(os_, (qs, ks, vs), go[idx])
    assert torch.equal(o[idx], os_) and torch.equal(gq[idx], gqs) and torch.equal(gk[idx], gks) and torch.equal(gv[idx], gvs)
    with torch.no_grad():
        o2 = ops.attention(q[:8], k[:8], 2.5 * v[:8], 0.125)
        assert _rel(o2, 2.5 * o[:8]) < 1e-5
        perm = torch.randperm(L, generator=g).to(dev)
        o3 = ops.attention(q[:8], k[:8][:, perm].contiguous(), v[:8][:, perm].contiguous(), 0.125)
        assert _rel(o3, o[:8]) < 1e-5


def test_linear_x6_full_size_row_independence_and_additivity():
    """M = 256 000 rows, 512 -> 2048 (the Transformer FFN): output rows equal those of a small call on the same rows (bitwise), the
    weight gradient is additive over row halves and the bias gradient is the column sum of the upstream gradient."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    M, Ci, Co = 256000, 512, 2048
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(M, Ci, generator=g).to(dev)
    w = (torch.randn(Co, Ci, generator=g) / Ci ** 0.5).to(dev).requires_grad_(True)
    b = torch.randn(Co, generator=g).to(dev).requires_grad_(True)
    gy = torch.randn(M, Co, generator=g).to(dev)
    y = ops.linear(x, w, b)
    rows = slice(128 * 700, 128 * 702)                      # two whole 128-row tiles
    with torch.no_grad():
        assert torch.equal(y[rows], ops.linear(x[rows].contiguous(), w, b))
    dw, db = torch.autograd.grad(y, (w, b), gy)
    h = M // 2
    y1, y2 = ops.linear(x[:h], w, b), ops.linear(x[h:], w, b)
    dw1, db1 = torch.autograd.grad(y1, (w, b), gy[:h])
    dw2, db2 = torch.autograd.grad(y2, (w, b), gy[h:])
    assert _rel(dw, dw1 + dw2) < 1e-5 and _rel(db, db1 + db2) < 1e-5
    assert _rel(db, gy.double().sum(0)) < 1e-5


def test_resnet_and_layernorm_full_size_sample_independence():
    """ResNet expert in eval mode at the benchmark shape (B=256, T=1000, C=122): a sample's logits do not depend on the batch it
    sits in (bitwise; convolution tiles never straddle samples).  LayerNorm at PatchTST's row count (3.9 M rows of 64): rows are
    independent of the launch shape."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    from models.ResNet import Model
    torch.manual_seed(0)
    m = Model(make_cfg(enc_in=122, seq_len=1000, num_class=3)).to(dev).eval()
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(256, 1000, 122, generator=g).to(dev)
    with torch.no_grad():
        full = m(x)
        part = m(x[[5, 77, 255]].contiguous())
    assert torch.equal(full[[5, 77, 255]], part)
    ln = torch.nn.LayerNorm(64).to(dev)
    h = torch.randn(256 * 122 * 125, 64, generator=g).to(dev)
    with torch.no_grad():
        y = ops.layer_norm(h, ln)
        assert torch.equal(y[1000003:1000003 + 70000], ops.layer_norm(h[1000003:1000003 + 70000].contiguous(), ln))
        assert _rel(y[:4096], torch.nn.functional.layer_norm(h[:4096].double(), (64,), ln.weight.double(), ln.bias.double())) < 2e-6


def test_weight_bounds_follow_the_optimizer():
    """The magnitude bound of a WEIGHT must be taken afresh at every call: the flat Adam kernel rewrites parameters through raw
    pointers (no version bump), so a cached bound would go stale -- here one Adam step with a huge learning rate grows the weight
    ~1000x, far beyond the 4x headroom between the scaled maximum (2^14) and fp16's overflow."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    from ign_hip.ddp import FlatAdam, FlatParamBucket
    torch.manual_seed(0)
    lin = torch.nn.Linear(64, 256).to(dev)
    bucket = FlatParamBucket(lin, 1)
    opt = FlatAdam(bucket, lr=50.0)
    x = torch.randn(40, 64, device=dev)
    for it in range(2):
        y = ops.linear(x, lin.weight, lin.bias)
        ref = torch.nn.functional.linear(x.double(), lin.weight.detach().double(), lin.bias.detach().double())
        assert torch.isfinite(y).all(), f"call {it}"
        assert _rel(y, ref) < 3e-6, f"call {it}"
        y.square().mean().backward()
        opt.step()
        bucket.zero_grad()
    assert float(lin.weight.detach().abs().max()) > 40.0          # the weight did grow far beyond its first bound
    y = ops.linear(x, lin.weight, lin.bias)
    ref = torch.nn.functional.linear(x.double(), lin.weight.detach().double(), lin.bias.detach().double())
    assert torch.isfinite(y).all() and _rel(y, ref) < 3e-6


def test_backward_operand_bounds_come_from_the_producers():
    """fp16 GEMM scaling in the backward of an encoder layer: every dL/dy operand carries a bound attached by the kernel that wrote
    it (LayerNorm backward, the dense layers' input-gradient epilogue, the attention backward, the activation's backward), so the
    only passes ign_absmax makes in a forward + backward are over the raw input and the (small) weights.  Each attached bound is
    checked against the tensor it describes (numerics: the parametrised kernel tests above run all of this on f16x3)."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops, _lib
    from models.eegcnn import _encoder_layer_forward
    if ops.GEMM_MATH != "f16x3":
        pytest.skip("needs the f16x3 arithmetic")
    torch.manual_seed(0)
    layer = torch.nn.TransformerEncoderLayer(d_model=64, nhead=4, dim_feedforward=128, dropout=0.0, batch_first=True).to(dev).train()
    x = torch.randn(4, 50, 64, device=dev)
    L = _lib.lib()
    calls, seen = [], []
    orig_absmax, orig_set = L.ign_absmax, ops.set_bound

    def spy_absmax(*a):
        calls.append(int(a[1]))
        return orig_absmax(*a)

    def spy_set(t, slot):
        seen.append((t, slot))
        return orig_set(t, slot)

    L.ign_absmax, ops.set_bound = spy_absmax, spy_set
    try:
        xin = x.clone().requires_grad_(True)
        out = _encoder_layer_forward(layer, xin, 4)
        (out * torch.randn_like(out)).sum().backward()
        torch.cuda.synchronize()
    finally:
        L.ign_absmax, ops.set_bound = orig_absmax, orig_set
    weights = [layer.self_attn.in_proj_weight, layer.self_attn.out_proj.weight, layer.linear1.weight, layer.linear2.weight]
    assert sorted(calls) == sorted([x.numel()] + [w.numel() for w in weights]), \
        f"ign_absmax passes over {calls} elements; expected the raw input and the four (small) weights only"
    assert len(seen) >= 10
    exact = 0
    for t, slot in seen:                                     # every attached bound bounds its tensor (4x headroom not needed here)
        tm = float(t.detach().abs().max())
        assert tm <= float(slot) * 1.14 + 1e-30, (tuple(t.shape), tm, float(slot))
        exact += tm == float(slot)
    # the bounds TAKEN by a kernel while it writes the tensor are the exact maximum (atomic maximum on the bit pattern): the four
    # dense outputs, their four input gradients, the two LayerNorm input gradients, the packed attention gradient
    assert exact >= 11, (exact, len(seen))
    assert all(torch.isfinite(p.grad).all() for p in layer.parameters()) and torch.isfinite(xin.grad).all()


def test_dense_layer_prologue_matches_the_per_layer_route_and_goes_stale_safely():
    """ops.prepare_linear_weights: bounds + packed planes of several weights in one scan and one packing launch.  (1) ops.linear on a
    prepared weight is bitwise the per-layer route; (2) an entry is consumed once; (3) an entry made before the parameters changed
    -- in place (version counter) or through the flat Adam kernel (raw pointers: _lib.PARAM_GENERATION) -- is NOT used."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops, _lib
    from ign_hip.ddp import FlatAdam, FlatParamBucket
    if ops.GEMM_MATH != "f16x3":
        pytest.skip("needs the f16x3 arithmetic")
    torch.manual_seed(0)
    lins = [torch.nn.Linear(64, 128).to(dev), torch.nn.Linear(128, 64).to(dev), torch.nn.Linear(64, 512, bias=False).to(dev)]
    xs = [torch.randn(50, 64, device=dev), torch.randn(50, 128, device=dev), torch.randn(7, 9, 64, device=dev)]

    def run(prep):
        outs = []
        if prep:
            ops.prepare_linear_weights([l.weight for l in lins])
            assert len(ops._PREPARED) == 3
        for l, x in zip(lins, xs):
            xr = x.clone().requires_grad_(True)
            y = ops.linear(xr, l.weight, l.bias)
            y.square().sum().backward()
            outs += [y.detach(), xr.grad, l.weight.grad.clone()]
            l.zero_grad(set_to_none=True)
        return outs

    a, b = run(False), run(True)
    assert not ops._PREPARED                                            # consumed
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # stale by an in-place update
    ops.prepare_linear_weights([l.weight for l in lins])
    with torch.no_grad():
        lins[0].weight.mul_(300.0)
    y = ops.linear(xs[0], lins[0].weight, lins[0].bias)
    ref = torch.nn.functional.linear(xs[0].double(), lins[0].weight.detach().double(), lins[0].bias.detach().double())
    assert torch.isfinite(y).all() and _rel(y, ref) < 3e-6
    # stale by the flat Adam kernel (no version bump)
    bucket = FlatParamBucket(lins[1], 1)
    opt = FlatAdam(bucket, lr=30.0)
    ops.linear(xs[1], lins[1].weight, lins[1].bias).square().mean().backward()
    ops.prepare_linear_weights([l.weight for l in lins])
    opt.step()
    bucket.zero_grad()
    y = ops.linear(xs[1], lins[1].weight, lins[1].bias)
    ref = torch.nn.functional.linear(xs[1].double(), lins[1].weight.detach().double(), lins[1].bias.detach().double())
    assert float(lins[1].weight.detach().abs().max()) > 20.0 and torch.isfinite(y).all() and _rel(y, ref) < 3e-6


@pytest.mark.parametrize("shape,Ci,Co,bias", [((4, 300, 512), 512, 128, True), ((3, 77, 256), 256, 64, False), ((130, 64), 64, 12, True),
                                              ((2, 50, 768), 768, 256, True)])
@pytest.mark.parametrize("gmath", ["f16x3", "bf16x6"])
def test_gelu_linear_against_float64(shape, Ci, Co, bias, gmath, monkeypatch):
    """ops.gelu_linear(u, W, b) = linear(gelu(u)): output, dL/du (the GELU derivative applied in the epilogue of the input-gradient
    GEMM where d_ff % 256 == 0 on the f16x3 arithmetic, torch's gelu_backward otherwise), dW, db against float64."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops, _lib
    monkeypatch.setattr(ops, "GEMM_MATH", gmath)
    g = torch.Generator().manual_seed(Ci + Co)
    u = torch.randn(*shape, generator=g) * 1.5
    w = torch.randn(Co, Ci, generator=g) / Ci ** 0.5
    b = torch.randn(Co, generator=g) * 0.1 if bias else None
    gz = torch.randn(*shape[:-1], Co, generator=g)
    ud, wd = u.double().requires_grad_(True), w.double().requires_grad_(True)
    bd = b.double().requires_grad_(True) if bias else None
    zd = F.linear(F.gelu(ud), wd, bd)
    (zd * gz.double()).sum().backward()
    ug, wg = u.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    bg = b.to(dev).requires_grad_(True) if bias else None
    L = _lib.lib()
    fused_calls = []
    orig = L.ign_linear_dgrad_gelu_h3
    L.ign_linear_dgrad_gelu_h3 = lambda *a: (fused_calls.append(1), orig(*a))[1]
    try:
        z = ops.gelu_linear(ug, wg, bg)
        (z * gz.to(dev)).sum().backward()
    finally:
        L.ign_linear_dgrad_gelu_h3 = orig
    assert bool(fused_calls) == (gmath == "f16x3" and Ci % 256 == 0)
    assert _rel(z, zd) < 3e-6
    assert _rel(ug.grad, ud.grad) < 5e-6
    assert _rel(wg.grad, wd.grad) < 5e-6
    if bias:
        assert _rel(bg.grad, bd.grad) < 5e-6
