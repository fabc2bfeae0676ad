"""SBM attention head on the fused kernels (ops.sbm_attention, include/ign_abi.h ign_sbm_attn_*): output and all six gradients
against a float64 torch restatement of IGN/model/Shapelet.py:117-131, at small and full size; O(B*F) memory; bitwise-reproducible
backward; the model routes through the kernels (eager, autocast, hipGraph).  Tolerance 1e-4 (north_star) through conftest.parity."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, make_cfg, parity, sd_from

pytestmark = pytest.mark.gpu

NAMES = ("q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias", "pos_embed.weight")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def _params(F_, dev, seed, pos_scale=3.0):
    g = torch.Generator().manual_seed(seed)
    wq, wk = torch.randn(16, 1, generator=g), torch.randn(16, 1, generator=g)
    bq, bk = torch.randn(16, generator=g) * 0.5, torch.randn(16, generator=g) * 0.5
    pos = torch.randn(F_, 16, generator=g) * pos_scale
    return [t.to(dev) for t in (wq, bq, wk, bk, pos)]


def _ref64(x, params, gout, chunk):
    """float64 restatement of SelfAttention + its gradients, in batch chunks so that no (B,F,F) tensor exceeds chunk*F*F."""
    ps = [p.detach().double().requires_grad_() for p in params]
    wq, bq, wk, bk, pos = ps
    outs, gxs = [], []
    for s in range(0, x.shape[0], chunk):
        xc = x[s:s + chunk].detach().double().requires_grad_()
        P = pos[:xc.shape[1]]
        q = xc[..., None] * wq[:, 0] + bq + P
        k = xc[..., None] * wk[:, 0] + bk + P
        att = torch.softmax(q @ k.transpose(1, 2) * 0.25, dim=-1)
        o = (att @ xc[..., None])[..., 0]
        (o * gout[s:s + chunk].double()).sum().backward()
        outs.append(o.detach())
        gxs.append(xc.grad)
        del q, k, att, o
    return torch.cat(outs), torch.cat(gxs), [p.grad for p in ps]


def _check(label, x, params, seed, chunk=64, pad=0):
    """`pad` > 0: the op reads x as the first F columns of a (B, F + pad) buffer (row pitch F + pad)."""
    from ign_hip import ops
    g = torch.Generator().manual_seed(seed + 1)
    gout = torch.randn(x.shape, generator=g).to(x.device)
    B, F_ = x.shape
    wide = torch.zeros(B, F_ + pad, device=x.device)
    wide[:, :F_] = x
    wide.requires_grad_()
    xin = wide[:, :F_]
    assert xin.stride(0) == F_ + pad
    ps = [p.detach().clone().requires_grad_() for p in params]
    out = ops.sbm_attention(xin, *ps)
    out.backward(gout)
    o64, gx64, gp64 = _ref64(x, params, gout, chunk)
    parity(f"{label}: out", out, o64, kind="elem", ref_is="float64 restatement")
    parity(f"{label}: grad x", wide.grad[:, :F_], gx64, kind="scale", ref_is="float64 restatement")
    assert not wide.grad[:, F_:].any()
    for n, p, r in zip(NAMES, ps, gp64):
        floor = 0.0
        if n == "k_proj.bias":
            # exactly zero in exact arithmetic (q_i.bk is constant along the softmax axis): judged against the scale of the
            # other head-parameter gradients, which is what its rounding is made of
            floor = max(float(gp64[i].abs().max()) for i in (0, 1, 2))
        parity(f"{label}: grad {n}", p.grad, r, kind="scale", floor=floor, ref_is="float64 restatement")
    return out, wide.grad[:, :F_], [p.grad for p in ps]


@pytest.mark.parametrize("B", [1, 3, 8, 64])
@pytest.mark.parametrize("F_", [1, 3, 31, 33, 360, 1000, 2440])
def test_op_matches_float64(B, F_):
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    g = torch.Generator().manual_seed(B * 7919 + F_)
    x = torch.randn(B, F_, generator=g).to(dev)
    # pos scale 3 where the softmax has keys to spread over; with F <= 3 it leaves every row one-hot (scores ~36 apart), the
    # parameter gradients fall below fp32 resolution and the torch fp32 composition itself misses them by up to 4x their size
    pos_scale = 3.0 if F_ >= 31 else 1.0
    _check(f"B{B} F{F_}", x, _params(F_, dev, seed=B + F_, pos_scale=pos_scale), seed=B * F_, chunk=16 if F_ > 1000 else 64)


def test_op_reads_a_row_pitch():
    """x a column slice of a wider buffer (row pitch F + 5), as p is when it comes out of the fused SBM node."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    x = torch.randn(40, 200, generator=torch.Generator().manual_seed(3)).to(dev)
    _check("pitch 205", x, _params(200, dev, seed=11), seed=12, pad=5)


def test_full_size_matches_float64():
    """B 256, F 2440 (InterpGN on CHISCO): 8 batch chunks x 39 row blocks and the 153-block reduction, all of it compared."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    x = torch.rand(256, 2440, generator=torch.Generator().manual_seed(21)).to(dev)
    _check("B256 F2440", x, _params(2440, dev, seed=22), seed=23, chunk=16)


def test_memory_is_linear_in_batch_and_features():
    """fwd + bwd at B 256, F 7320 (SBM / LTS on CHISCO): one (B,F,F) fp32 tensor would be 54.9 GB; the head stays under 256 MB
    over its inputs (o, lse, dx, the upstream gradient and the 8-chunk workspace are ~40 MB)."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    B, F_ = 256, 7320
    x = torch.rand(B, F_, device=dev).requires_grad_()
    ps = [p.requires_grad_() for p in _params(F_, dev, seed=5, pos_scale=1.0)]
    gout = torch.randn(B, F_, device=dev)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = ops.sbm_attention(x, *ps)
    out.backward(gout)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert extra < 256 << 20, f"{extra / 2**20:.1f} MB"
    assert torch.isfinite(x.grad).all() and all(torch.isfinite(p.grad).all() for p in ps)


def test_backward_is_bitwise_reproducible():
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    x0 = torch.rand(96, 1000, generator=torch.Generator().manual_seed(8)).to(dev)
    gout = torch.randn(96, 1000, generator=torch.Generator().manual_seed(9)).to(dev)
    params = _params(1000, dev, seed=10)
    runs = []
    for _ in range(2):
        x = x0.clone().requires_grad_()
        ps = [p.clone().requires_grad_() for p in params]
        out = ops.sbm_attention(x, *ps)
        out.backward(gout)
        runs.append([out.detach(), x.grad] + [p.grad for p in ps])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_no_grad_forward_equals_the_autograd_forward():
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import ops
    x = torch.rand(5, 77, device=dev)
    ps = [p.requires_grad_() for p in _params(77, dev, seed=2)]
    with torch.no_grad():
        a = ops.sbm_attention(x, *ps)
    b = ops.sbm_attention(x, *ps)
    assert b.requires_grad and not a.requires_grad
    assert torch.equal(a, b.detach())


def _sbm(dev, **kw):
    from models.Shapelet import ShapeBottleneckModel
    g = golden("sbm_attention")
    k = int(g["num_shapelet"])
    m = ShapeBottleneckModel(make_cfg(sbm_cls="attention", **kw), [k] * 6, [0.05, 0.1, 0.2, 0.3, 0.5, 0.8])
    m.load_state_dict(sd_from(g))
    return m.to(dev).train(), g


def _no_sdpa(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("F.scaled_dot_product_attention called: the head did not take the fused kernels")
    orig = F.scaled_dot_product_attention
    monkeypatch.setattr(F, "scaled_dot_product_attention", boom)
    return orig


def test_model_routes_through_the_kernels_and_matches_the_fixture(monkeypatch):
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    _no_sdpa(monkeypatch)
    m, g = _sbm(dev)
    x, y = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["y"]).to(dev)
    out, info = m(x)
    loss = F.cross_entropy(out, y) + info.loss.mean()
    loss.backward()
    parity("out", out, g["out"], kind="elem", f64=g.get("out64"))
    parity("train_loss", loss, g["train_loss"], kind="elem")
    gmax = max(float(np.abs(g[k]).max()) for k in g if k.startswith("grad."))
    for n, p in m.named_parameters():
        ref = g["grad." + n]
        if float(np.abs(ref).max()) < 1e-5 * gmax:          # attention.k_proj.bias: zero in exact arithmetic
            assert float(p.grad.abs().max()) < 1e-5 * gmax, n
            continue
        parity("grad." + n, p.grad, ref, kind="scale", floor=1e-4 * gmax, f64=g.get("grad64." + n))
    m.eval()
    with torch.no_grad():
        oe, _ = m(x)
    assert torch.isfinite(oe).all()


def test_model_inside_autocast_runs_the_fp32_kernels(monkeypatch):
    """Inside torch.autocast(cuda, bf16) the head runs the same fp32 kernels and returns fp32; the model output tracks the torch
    composition under autocast at bf16 tolerance."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    sdpa = _no_sdpa(monkeypatch)
    m, g = _sbm(dev)
    x = torch.from_numpy(g["x"]).to(dev)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        out, info = m(x)
        att = m.attention(info.p)
        assert att.dtype == torch.float32
        a = m.attention
        pos = a.pos_embed(torch.arange(info.p.shape[1], device=dev))
        q = a.q_proj(info.p.unsqueeze(-1)) + pos
        k = a.k_proj(info.p.unsqueeze(-1)) + pos
        ref_att = sdpa(q, k, info.p.unsqueeze(-1)).squeeze(-1)
        ref = m.output_layer(ref_att)
    fp32 = torch.from_numpy(g["out"]).to(dev)
    parity("autocast head vs fp32 fixture head input", att, m.attention(info.p.detach()), kind="elem",
           ref_is="the same kernels outside autocast")
    scale = max(1.0, float(ref.detach().float().abs().max()))
    assert float((out.float() - ref.float()).abs().max()) < 3e-2 * scale
    assert float((att - ref_att.float()).abs().max()) < 3e-2 * max(1.0, float(ref_att.float().abs().max()))
    assert float((out.float() - fp32).abs().max()) < 5e-2 * max(1.0, float(fp32.abs().max()))


def test_graphed_sbm_attention_step_equals_eager():
    """One SBM step with the attention head (fused SBM node, head kernels, backward, capturable flat Adam) captured as a hipGraph
    and replayed on 3 batches walks the eager parameter trajectory (mirrors test_gpu_models.test_graphed_train_step_equals_eager)."""
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa
    from ign_hip.ddp import FlatAdam, FlatParamBucket
    from ign_hip.graph import GraphedTrainStep
    from models.Shapelet import ShapeBottleneckModel
    torch.manual_seed(0)
    base = ShapeBottleneckModel(make_cfg(sbm_cls="attention"))
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(8, 100, 6, generator=g).to(dev) for _ in range(4)]
    ys = [(torch.arange(8) % 4).to(dev) for _ in range(4)]
    finals = {}
    for mode in ("eager", "graph"):
        model = copy.deepcopy(base).to(dev).train()
        bucket = FlatParamBucket(model, 1)
        opt = FlatAdam(bucket, lr=5e-3, capturable=(mode == "graph"))

        def step(x, y, model=model, bucket=bucket, opt=opt):
            out, info = model(x)
            loss = F.cross_entropy(out, y) + info.loss.mean()
            loss.backward()
            opt.step()
            bucket.zero_grad()
            return loss.detach()

        if mode == "graph":
            sd = copy.deepcopy(model.state_dict())
            stepper = GraphedTrainStep(step, (xs[0], ys[0]), warmup=2)
            model.load_state_dict(sd)
            opt.exp_avg.zero_(); opt.exp_avg_sq.zero_(); opt.step_dev.zero_()
        else:
            stepper = step
        losses = [float(stepper(x, y)) for x, y in zip(xs[1:], ys[1:])]
        torch.cuda.synchronize()
        finals[mode] = (losses, {k: v.detach().clone() for k, v in model.state_dict().items()})
    for a, b in zip(finals["eager"][0], finals["graph"][0]):
        assert a == a and abs(a - b) <= 1e-6 * max(1.0, abs(a)), (finals["eager"][0], finals["graph"][0])
    for k, v in finals["eager"][1].items():
        w = finals["graph"][1][k]
        if v.dtype.is_floating_point:
            assert float((v - w).abs().max()) <= 1e-6 * max(1.0, float(v.abs().max())), k
    assert finals["eager"][1]["attention.pos_embed.weight"].ne(base.state_dict()["attention.pos_embed.weight"].to(dev)).any()
