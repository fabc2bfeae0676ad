"""AdamW, the scheduled tick, the EMA update and the buffer exchange on the GPU (csrc/ign_optim.hip): neutral settings against the
existing device-count Adam bit for bit, five scheduled AdamW steps under a chunk mask against the float64 rule
(utils.optim_rule.adamw_reference), the learning rate and EMA decay the tick leaves on the device, bounds, ign_ema_update,
ign_swap_flat, non-finite gradients, and FlatAdam end to end against torch.optim.AdamW with parameter groups."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from conftest import parity

pytestmark = pytest.mark.gpu

# the sweep of test_gpu_clip.py's Adam tests across the 16-byte tail and a block edge (1024 floats per block): tail only, tail of 3,
# one vector + 1, one mask chunk exactly, the last lane of a block, one element into the second block, several blocks plus one
NS = (1, 3, 5, 64, 1023, 1025, 4097)
BUF, FULL = 4104, 4100                          # FULL: no tail; BUF - FULL floats behind it that no run may touch
BASE, FLOOR, WD, COEF = 5e-3, 5e-4, 0.05, 0.37
W, S, STEPS = 2, 5, 5                           # warm-up for s = 1, base at s = 2, the cosine down to FLOOR at s = 5
B1, B2, EPS = 0.9, 0.999, 1e-8
_cache = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _mods():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    from utils import optim_rule
    return _lib, optim_rule


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _inputs():
    """host p, m, v of BUF floats and one gradient per step: the same for every test"""
    if "inputs" not in _cache:
        gen = torch.Generator().manual_seed(31)
        _cache["inputs"] = (torch.randn(BUF, generator=gen), torch.randn(BUF, generator=gen), torch.rand(BUF, generator=gen),
                            [torch.randn(BUF, generator=gen) for _ in range(STEPS)])
    return _cache["inputs"]


def _chunk_mask(n=BUF):
    """decay [0, 64), none [64, 192), decay [192, n): the segments start and end at 64-float boundaries that are no block edges"""
    chunks = torch.ones((n + 63) // 64, dtype=torch.uint8)
    chunks[1:3] = 0
    return chunks


def _elem_mask(n):
    i = np.arange(n)
    return (i < 64) | (i >= 192)


def _run(lib, dev, n, steps, wd=WD, mask="chunks", kind=1, warmup=W, floor=FLOOR, total=S, ema=0.0, clip=False):
    """`steps` calls of ign_adamw_step_dev over the first n floats of fresh copies of the inputs
    -> (p, m, v on the host, [hp_dev after each step], step count)"""
    p0, m0, v0, gs = _inputs()
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    mk = _chunk_mask().to(dev) if mask == "chunks" else None
    coef = torch.tensor([COEF], device=dev) if clip else None
    step_dev, hp = torch.zeros(1, device=dev, dtype=torch.int32), torch.zeros(4, device=dev)
    hps = []
    for k in range(steps):
        g = gs[k].to(dev)
        lib.check(lib.lib().ign_adamw_step_dev(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, B1, B2, EPS, wd, _ptr(mk), kind, BASE, warmup,
                                               floor, total, ema, _ptr(step_dev), _ptr(hp), _ptr(coef), lib.stream()),
                  "ign_adamw_step_dev")
        hps.append(hp.cpu().numpy().copy())
    return p.cpu(), m.cpu(), v.cpu(), hps, int(step_dev)


def _adam_dev(lib, dev, n, steps, clip):
    """the existing device-count Adam from the same start, at lr = BASE"""
    p0, m0, v0, gs = _inputs()
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    coef = torch.tensor([COEF], device=dev)
    step_dev, bc = torch.zeros(1, device=dev, dtype=torch.int32), torch.zeros(2, device=dev)
    for k in range(steps):
        g = gs[k].to(dev)
        args = [_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, BASE, B1, B2, EPS, _ptr(step_dev), _ptr(bc)]
        entry = "ign_adam_step_clip_dev" if clip else "ign_adam_step_dev"
        lib.check(getattr(lib.lib(), entry)(*(args + ([_ptr(coef)] if clip else [])), lib.stream()), entry)
    return p.cpu(), m.cpu(), v.cpu(), bc.cpu().numpy()


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# ---------------------------------------------------------------- neutral settings are the old path
@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("n", NS)
def test_neutral_settings_are_the_device_count_adam_bit_for_bit(n, clip):
    dev = _dev()
    lib, _ = _mods()
    for mask in ("chunks", None):                  # weight_decay 0 skips the multiply whatever the mask says
        p, m, v, hps, count = _run(lib, dev, n, 3, wd=0.0, mask=mask, kind=0, warmup=0, floor=0.0, total=0, clip=clip)
        q, mq, vq, bc = _adam_dev(lib, dev, n, 3, clip)
        assert count == 3
        assert torch.equal(p, q) and torch.equal(m, mq) and torch.equal(v, vq)
        assert not torch.equal(p[:n], _inputs()[0][:n])
        assert hps[-1][0] == bc[0] and hps[-1][1] == bc[1] and hps[-1][2] == np.float32(BASE)


# ---------------------------------------------------------------- five scheduled steps against float64
def _reference(R, n, wd):
    key = ("ref", n, wd)
    if key not in _cache:
        p0, m0, v0, gs = _inputs()
        spec = R.LrSchedule("cosine", W, FLOOR)
        p, m, v = p0[:n].double().numpy(), m0[:n].double().numpy(), v0[:n].double().numpy()
        for s in range(1, STEPS + 1):
            p, m, v = R.adamw_reference(p, gs[s - 1][:n].double().numpy(), m, v, lr=R.lr_at(spec, BASE, S, s), step=s,
                                        betas=(B1, B2), eps=EPS, weight_decay=wd, decay=_elem_mask(n))
        _cache[key] = (p, m, v)
    return _cache[key]


@pytest.mark.parametrize("n", NS)
def test_five_adamw_steps_with_cosine_and_warmup_against_float64(n):
    dev = _dev()
    lib, R = _mods()
    spec = R.LrSchedule("cosine", W, FLOOR)
    p, m, v, hps, count = _run(lib, dev, n, STEPS)
    assert count == STEPS
    for s, hp in enumerate(hps, 1):
        want = np.float32(R.lr_at(spec, BASE, S, s))
        print(f"n={n} step {s}: lr on the device {hp[2]!r}, host rule {want!r}")
        assert _ulps(hp[2], want) <= 1, s
    assert hps[0][2] == np.float32(BASE / 2) and hps[1][2] == np.float32(BASE)       # the warm-up and its end: exact
    rp, rm, rv = _reference(R, n, WD)
    for what, got, ref in (("p", p, rp), ("m", m, rm), ("v", v, rv)):
        parity(f"adamw {what} n={n}", got[:n], ref)
    # an undecayed segment takes the path of weight_decay = 0 to the bit; a decayed one does not
    q = _run(lib, dev, n, STEPS, wd=0.0)[0]
    assert torch.equal(p[64:192], q[64:192])
    assert not torch.equal(p[:min(n, 64)], q[:min(n, 64)])
    if n > 192:
        assert not torch.equal(p[192:n], q[192:n])
        # a null mask decays everything: the same bits where the mask said decay, others where it did not
        a = _run(lib, dev, n, STEPS, mask=None)[0]
        assert torch.equal(a[:64], p[:64]) and torch.equal(a[192:], p[192:]) and not torch.equal(a[64:192], p[64:192])


@pytest.mark.parametrize("n", NS)
def test_clipped_adamw_reads_the_gradient_times_the_coefficient(n):
    dev = _dev()
    lib, R = _mods()
    p0, m0, v0, gs = _inputs()
    spec = R.LrSchedule("cosine", W, FLOOR)
    c = float(torch.tensor(COEF, dtype=torch.float32))
    rp, rm, rv = p0[:n].double().numpy(), m0[:n].double().numpy(), v0[:n].double().numpy()
    for s in range(1, 4):
        rp, rm, rv = R.adamw_reference(rp, gs[s - 1][:n].double().numpy() * c, rm, rv, lr=R.lr_at(spec, BASE, S, s), step=s,
                                       betas=(B1, B2), eps=EPS, weight_decay=WD, decay=_elem_mask(n))
    p, m, v, _, _ = _run(lib, dev, n, 3, clip=True)
    for what, got, ref in (("p", p, rp), ("m", m, rm), ("v", v, rv)):
        parity(f"adamw clip {what} n={n}", got[:n], ref)


# ---------------------------------------------------------------- bounds
@pytest.mark.parametrize("n", NS + (4, 1024))
def test_a_run_over_n_is_the_prefix_of_the_full_run_and_writes_nothing_past_n(n):
    dev = _dev()
    lib, _ = _mods()
    if "full" not in _cache:
        _cache["full"] = _run(lib, dev, FULL, 1)[:3]
    p0, m0, v0, _ = _inputs()
    for what, got, full, init in zip("pmv", _run(lib, dev, n, 1)[:3], _cache["full"], (p0, m0, v0)):
        assert torch.equal(got[:n], full[:n]), what
        assert torch.equal(got[n:], init[n:]), what
        assert not torch.equal(got[:n], init[:n]), what


# ---------------------------------------------------------------- EMA
def _tick(lib, dev, hp, step_dev, ema):
    """one scheduled tick (an AdamW step over a scratch vector): hp = [.., .., lr_t, d_t] of the next step"""
    z = [torch.zeros(4, device=dev) for _ in range(4)]
    lib.check(lib.lib().ign_adamw_step_dev(*[_ptr(t) for t in z], 4, B1, B2, EPS, 0.0, None, 0, BASE, 0, 0.0, 0, ema, _ptr(step_dev),
                                           _ptr(hp), None, lib.stream()), "ign_adamw_step_dev")


@pytest.mark.parametrize("n", NS)
def test_ema_update_against_float64_and_the_decay_warm_up(n):
    dev = _dev()
    lib, R = _mods()
    p0, e0, _, gs = _inputs()
    ema, ref = e0.to(dev), e0[:n].double().numpy()
    step_dev, hp = torch.zeros(1, device=dev, dtype=torch.int32), torch.zeros(4, device=dev)
    for s in range(1, 6):
        p = (p0 + 0.1 * gs[s - 1]).to(dev)           # the parameters move from step to step
        _tick(lib, dev, hp, step_dev, 0.999)
        assert float(hp[3]) == float(np.float32(R.ema_decay_at(0.999, s))) == float(np.float32((1 + s) / (10 + s))), s
        lib.check(lib.lib().ign_ema_update(_ptr(ema), _ptr(p), n, _ptr(hp), lib.stream()), "ign_ema_update")
        ref = R.ema_reference(ref, p[:n].double().cpu().numpy(), 0.999, s)
    parity(f"ema n={n}", ema[:n], ref)
    assert torch.equal(ema[n:].cpu(), e0[n:])                                     # nothing past n
    # a decay below the warm-up value is taken as it is
    _tick(lib, dev, hp, step_dev, 0.25)
    assert int(step_dev) == 6 and float(hp[3]) == 0.25
    # p == ema: the average keeps its bits
    same = ema.clone()
    before = ema.clone()
    lib.check(lib.lib().ign_ema_update(_ptr(ema), _ptr(same), n, _ptr(hp), lib.stream()), "ign_ema_update")
    assert torch.equal(ema, before)


# ---------------------------------------------------------------- swap
@pytest.mark.parametrize("n", NS + (4100,))
def test_swap_flat_exchanges_and_restores(n):
    dev = _dev()
    lib, _ = _mods()
    a0, b0, _, _ = _inputs()
    a, b = a0.to(dev), b0.to(dev)
    lib.check(lib.lib().ign_swap_flat(_ptr(a), _ptr(b), n, lib.stream()), "ign_swap_flat")
    assert torch.equal(a[:n].cpu(), b0[:n]) and torch.equal(b[:n].cpu(), a0[:n])
    assert torch.equal(a[n:].cpu(), a0[n:]) and torch.equal(b[n:].cpu(), b0[n:])
    lib.check(lib.lib().ign_swap_flat(_ptr(a), _ptr(b), n, lib.stream()), "ign_swap_flat")
    assert torch.equal(a.cpu(), a0) and torch.equal(b.cpu(), b0)


# ---------------------------------------------------------------- through FlatAdam
class _Net(torch.nn.Module):
    """weights of 130 and 70 floats (three and two mask chunks) that decay, biases and a LayerNorm that do not"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(5)
        self.a, self.norm, self.b = torch.nn.Linear(13, 10), torch.nn.LayerNorm(10), torch.nn.Linear(10, 7)

    def forward(self, x):
        return self.b(self.norm(torch.tanh(self.a(x))))


def test_flat_adam_with_decay_schedule_and_ema_against_torch_adamw_in_float64():
    dev = _dev()
    lib, R = _mods()
    from ign_hip.ddp import FlatAdam, FlatParamBucket
    net = _Net().to(dev)
    ref = copy.deepcopy(net).double()
    bucket = FlatParamBucket(net, 1)
    opt = FlatAdam(bucket, lr=BASE, weight_decay=WD, schedule=f"cosine,warmup={W},min={FLOOR}", total_steps=S, ema=0.9)
    assert opt.decay_mask.tolist() == [1, 1, 1, 0, 0, 0, 1, 1, 0]
    decay = [p for k, p in ref.named_parameters() if R.decays(k, p)]
    rest = [p for k, p in ref.named_parameters() if not R.decays(k, p)]
    assert len(decay) == 2 and len(rest) == 4
    opt_ref = torch.optim.AdamW([dict(params=decay, weight_decay=WD), dict(params=rest, weight_decay=0.0)], lr=BASE)
    avg = [q.detach().clone() for q in ref.parameters()]
    gen = torch.Generator().manual_seed(6)
    for s in range(1, STEPS + 1):
        for group in opt_ref.param_groups:
            group["lr"] = opt.lr_at(s)
        for p, q in zip(net.parameters(), ref.parameters()):      # the same gradient for both, as autograd would leave it
            g = torch.randn(p.shape, generator=gen).to(dev)
            p.grad, q.grad = g, g.double()
        opt.step()
        opt.ema_update()
        opt.zero_grad()
        opt_ref.step()
        opt_ref.zero_grad()
        d = R.ema_decay_at(0.9, s)
        avg = [e + (1.0 - d) * (q.detach() - e) for e, q in zip(avg, ref.parameters())]
        assert _ulps(float(opt.hp_dev[2]), opt.lr_at(s)) <= 1 and int(opt.step_dev) == s
    live = [p.detach().clone() for p in net.parameters()]
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        parity(f"FlatAdam AdamW {k}", p, q)
    opt.swap_ema()                                  # the model now holds the average, through the same views
    for (k, p), e, l in zip(net.named_parameters(), avg, live):
        parity(f"FlatAdam EMA {k}", p, e)
        assert not torch.equal(p, l), k
    opt.swap_ema()
    for p, l in zip(net.parameters(), live):
        assert torch.equal(p, l)


class _Three(torch.nn.Module):
    """test_gpu_clip.py's three parameters of 1, 130 and 4 099 floats"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((1,), (130,), (4099,))])


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_non_finite_gradient_lands_where_torch_adamw_puts_it(bad):
    """the NaN / finite masks of clip_grad_norm_ + torch.optim.AdamW in fp32 on the GPU (the comparison of test_gpu_clip.py)"""
    dev = _dev()
    _mods()
    from ign_hip.ddp import FlatAdam, FlatParamBucket
    net = _Three().to(dev)
    ref = copy.deepcopy(net)
    bucket = FlatParamBucket(net, 1)
    opt, opt_ref = FlatAdam(bucket, lr=BASE, weight_decay=WD), torch.optim.AdamW(ref.parameters(), lr=BASE, weight_decay=WD)
    opt.decay_mask.fill_(1)                          # torch decays every parameter of the group: so does this run
    for step in range(2):
        gen = torch.Generator().manual_seed(100 + step)
        gs = [torch.randn(s, generator=gen) for s in ((1,), (130,), (4099,))]
        if step == 1:
            gs[1][7] = bad
        for p, q, g in zip(net.ps, ref.ps, gs):
            p.grad, q.grad = g.to(dev), g.to(dev).clone()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=0.5)
        opt_ref.step()
        opt.step(max_norm=0.5)
        opt.zero_grad()
    for i, (p, q, off) in enumerate(zip(net.ps, ref.ps, bucket.offsets)):
        n = p.numel()
        mine = (p.detach().reshape(-1), opt.exp_avg[off:off + n], opt.exp_avg_sq[off:off + n])
        theirs = (q.detach().reshape(-1), opt_ref.state[q]["exp_avg"].reshape(-1), opt_ref.state[q]["exp_avg_sq"].reshape(-1))
        for what, a, b in zip(("param", "exp_avg", "exp_avg_sq"), mine, theirs):
            assert torch.equal(torch.isnan(a), torch.isnan(b)), (i, what)
            assert torch.equal(torch.isfinite(a), torch.isfinite(b)), (i, what)
    assert sum(int(torch.isnan(p).sum()) for p in net.ps) == (1 if bad == float("inf") else 1 + 130 + 4099)
