"""Gradient clipping and accumulation on the flat gradient buffer, on the GPU: ign_grad_norm_clip against a float64 norm, the
clipped FlatAdam step against clip_grad_norm_ + torch.optim.Adam, non-finite gradients, the accumulating gather against autograd's
own accumulation, and the harness (eager and --hipgraph) with clip 0.5 and accumulation 2."""
import copy
import ctypes
import os

import pytest
import torch

from conftest import parity

pytestmark = pytest.mark.gpu

# floats per stage-1 block of ign_grad_norm_clip (NORM_SLICE in csrc/ign_optim.hip); the workspace is 4 header floats + one partial
# per slice, which is how the test below pins the constant
SLICE = 4096
# 64: one aligned slot (one partial, mostly tail).  4160 = 4096 + 64: a second slice of 64 floats.  65 * 4096 - 3996: 65 partials
# -- one more than a wave holds, so the second stage's lane 0 of wave 1 has work -- the last slice 100 floats long.
LENGTHS = (64, 4160, 64 * SLICE + 100)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _lib():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    return _lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _wide_values(n, seed):
    """magnitudes log-uniform over 1e-4 .. 1e3, random signs"""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 7.0 - 4.0)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float()


def _norm_clip(lib, buf, max_norm, ws=None):
    n = buf.numel()
    nbytes = lib.lib().ign_grad_norm_workspace_bytes(n)
    assert nbytes == 4 * (4 + (n + SLICE - 1) // SLICE)
    if ws is None:
        ws = torch.zeros(nbytes // 4, device=buf.device)          # zero-filled once; every call hands the counter back at zero
    out2 = torch.full((2,), -1.0, device=buf.device)
    lib.check(lib.lib().ign_grad_norm_clip(_ptr(buf), n, max_norm, _ptr(out2), _ptr(ws), lib.stream()), "ign_grad_norm_clip")
    return out2, ws


@pytest.mark.parametrize("n", LENGTHS)
def test_grad_norm_and_coefficient_against_float64(n):
    dev, lib = _dev(), _lib()
    buf = _wide_values(n, n).to(dev)
    ref = float(buf.double().square().sum().sqrt())
    for which, max_norm in (("above", 2.0 * ref), ("below", 0.01 * ref)):
        out2, ws = _norm_clip(lib, buf, max_norm)
        coef = min(1.0, max_norm / (ref + 1e-6))
        print(f"n={n} max_norm {which}: norm {float(out2[0])!r} vs {ref!r}, coefficient {float(out2[1])!r} vs {coef!r}")
        parity(f"grad_norm n={n} {which}", out2[:1], torch.tensor([ref], dtype=torch.float64))
        parity(f"clip_coef n={n} {which}", out2[1:], torch.tensor([coef], dtype=torch.float64))
        if which == "above":
            assert float(out2[1]) == 1.0                           # exactly 1: Adam then reads g * 1
        else:
            assert float(out2[1]) < 1.0
        again, _ = _norm_clip(lib, buf, max_norm, ws)             # same workspace: the ticket counter came back at zero
        assert torch.equal(out2, again)
        fresh, _ = _norm_clip(lib, buf, max_norm)
        assert torch.equal(out2, fresh)


def test_zero_padding_between_the_slots_changes_nothing():
    dev, lib = _dev(), _lib()
    vals = _wide_values(130, 3).to(dev)
    padded = torch.zeros(4160, device=dev)
    padded[:1], padded[64:64 + 129] = vals[:1], vals[1:]
    out2, _ = _norm_clip(lib, padded, 0.5)
    ref = float(vals.double().square().sum().sqrt())
    parity("grad_norm padded", out2[:1], torch.tensor([ref], dtype=torch.float64))


# ---------------------------------------------------------------- clipped Adam
class _Three(torch.nn.Module):
    """three parameters of 1, 130 and 4 099 floats: slots at 0, 64 and 256 of a 4 416-float buffer, zero padding in between"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((1,), (130,), (4099,))])


def _grads(step, scale=1.0):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(s, generator=g) * scale for s in ((1,), (130,), (4099,))]


# steps 0 and 1 are clipped (norm ~ 65 >> 0.5), step 2 is not (norm ~ 0.065: coefficient exactly 1)
STEP_SCALES = (1.0, 1.0, 1e-3)


@pytest.mark.parametrize("capturable", [False, True], ids=["host count", "capturable"])
def test_clipped_flat_adam_against_clip_grad_norm_and_torch_adam_in_float64(capturable):
    dev = _dev()
    _lib()
    from ign_hip.ddp import FlatAdam, FlatParamBucket
    net = _Three().to(dev)
    ref = copy.deepcopy(net).double()
    bucket = FlatParamBucket(net, 1)
    assert bucket.offsets == [0, 64, 256] and bucket.flat_grad.numel() == 4416
    opt, opt_ref = FlatAdam(bucket, lr=5e-3, capturable=capturable), torch.optim.Adam(ref.parameters(), lr=5e-3)
    for step, scale in enumerate(STEP_SCALES):
        gs = _grads(step, scale)
        for p, q, g in zip(net.ps, ref.ps, gs):
            p.grad, q.grad = g.to(dev), g.to(dev).double()
        norm_ref = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=0.5)
        opt_ref.step()
        opt.step(max_norm=0.5)
        opt.zero_grad()
        parity(f"last_grad_norm step {step}", opt.last_grad_norm.reshape(1), norm_ref.reshape(1))
        assert (float(opt.norm_dev[1]) == 1.0) == (scale < 1.0)
    for i, (p, q) in enumerate(zip(net.ps, ref.ps)):
        err = float((p.double() - q).abs().max())
        print(f"parameter {i}: max |hip - float64| = {err:.3e}")
        assert err < 1e-5, i                    # the bound of test_head_linear_gate_and_flat_adam_vs_torch


@pytest.mark.parametrize("capturable", [False, True], ids=["host count", "capturable"])
def test_step_with_max_norm_none_is_bitwise_step(capturable):
    dev = _dev()
    _lib()
    from ign_hip.ddp import FlatAdam, FlatParamBucket
    state = []
    for kw in ({}, {"max_norm": None}):
        net = _Three().to(dev)
        bucket = FlatParamBucket(net, 1)
        opt = FlatAdam(bucket, lr=5e-3, capturable=capturable)
        for step in range(3):
            for p, g in zip(net.ps, _grads(step)):
                p.grad = g.to(dev)
            opt.step(**kw)
            opt.zero_grad()
        state.append((opt.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()))
    for a, b in zip(*state):
        assert torch.equal(a, b)


@pytest.mark.parametrize("capturable", [False, True], ids=["host count", "capturable"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_non_finite_gradient_lands_where_torch_puts_it(bad, capturable):
    """inf: norm inf, coefficient 0, inf * 0 = NaN in that element alone, every other gradient 0.  NaN: NaN coefficient, everything
    NaN.  Reference: clip_grad_norm_ + torch.optim.Adam in fp32 on the GPU."""
    dev = _dev()
    _lib()
    from ign_hip.ddp import FlatAdam, FlatParamBucket
    net = _Three().to(dev)
    ref = copy.deepcopy(net)
    bucket = FlatParamBucket(net, 1)
    opt, opt_ref = FlatAdam(bucket, lr=5e-3, capturable=capturable), torch.optim.Adam(ref.parameters(), lr=5e-3)
    for step in range(2):
        gs = _grads(step)
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
    nan_params = sum(int(torch.isnan(p).sum()) for p in net.ps)
    assert nan_params == (1 if bad == float("inf") else 1 + 130 + 4099)


def test_clip_scales_the_gradients_themselves():
    dev = _dev()
    _lib()
    from ign_hip.ddp import FlatParamBucket
    net = _Three().to(dev)
    ref = copy.deepcopy(net).double()
    bucket = FlatParamBucket(net, 1)
    for p, q, g in zip(net.ps, ref.ps, _grads(0)):
        p.grad, q.grad = g.to(dev), g.to(dev).double()
    norm_ref = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=0.5)
    norm = bucket.clip_(0.5)
    assert norm.dim() == 0 and norm.is_cuda
    parity("clip_ norm", norm.reshape(1), norm_ref.reshape(1))
    for i, (p, q, v) in enumerate(zip(net.ps, ref.ps, bucket.views)):
        assert p.grad is v
        parity(f"clip_ grad {i}", p.grad, q.grad)


# ---------------------------------------------------------------- the four Adam entry points, called directly
ADAM_ENTRIES = ("ign_adam_step", "ign_adam_step_clip", "ign_adam_step_dev", "ign_adam_step_clip_dev")
# tail only, tail of 3, no tail, tail of 1, the last lane of a block, exactly one block (the grid formula adds an empty one), one
# element into the second block, several blocks plus a tail
ADAM_NS = (1, 3, 4, 5, 1023, 1024, 1025, 4099)
ADAM_BUF, ADAM_FULL = 4104, 4100                # 4100: no tail, every element goes through the 16-byte body
ADAM_LR, ADAM_COEF = 5e-3, 0.37
_adam_cache = {}


def _adam_inputs():
    """host (p, g, m, v) of ADAM_BUF floats, the same for every test"""
    if "inputs" not in _adam_cache:
        gen = torch.Generator().manual_seed(29)
        _adam_cache["inputs"] = (torch.randn(ADAM_BUF, generator=gen), torch.randn(ADAM_BUF, generator=gen),
                                 torch.randn(ADAM_BUF, generator=gen), torch.rand(ADAM_BUF, generator=gen))
    return _adam_cache["inputs"]


def _adam_run(lib, dev, entry, n, steps):
    """`steps` calls of `entry` over the first n floats of fresh copies of the inputs -> (p, m, v) on the host"""
    p, g, m, v = (t.to(dev) for t in _adam_inputs())
    coef = torch.tensor([ADAM_COEF], device=dev)
    step_dev, bc_dev = torch.zeros(1, device=dev, dtype=torch.int32), torch.zeros(2, device=dev)
    for k in range(steps):
        args = [_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, ADAM_LR, 0.9, 0.999, 1e-8]
        args += [_ptr(step_dev), _ptr(bc_dev)] if entry.endswith("_dev") else [k + 1]
        if "_clip" in entry:
            args.append(_ptr(coef))
        lib.check(getattr(lib.lib(), entry)(*args, lib.stream()), entry)
    if entry.endswith("_dev"):
        assert int(step_dev) == steps
    return p.cpu(), m.cpu(), v.cpu()


@pytest.mark.parametrize("n", ADAM_NS)
@pytest.mark.parametrize("entry", ADAM_ENTRIES)
def test_adam_entry_over_n_is_the_prefix_of_the_full_run_and_writes_nothing_past_n(entry, n):
    dev, lib = _dev(), _lib()
    if entry not in _adam_cache:
        _adam_cache[entry] = _adam_run(lib, dev, entry, ADAM_FULL, 1)
    p0, _, m0, v0 = _adam_inputs()
    for what, got, full, init in zip("pmv", _adam_run(lib, dev, entry, n, 1), _adam_cache[entry], (p0, m0, v0)):
        assert torch.equal(got[:n], full[:n]), what
        assert torch.equal(got[n:], init[n:]), what
        assert not torch.equal(got[:n], init[:n]), what


@pytest.mark.parametrize("n", ADAM_NS)
@pytest.mark.parametrize("entry", ADAM_ENTRIES)
def test_adam_entry_three_steps_against_torch_adam_in_float64(entry, n):
    dev, lib = _dev(), _lib()
    p0, g0, m0, v0 = _adam_inputs()
    q = torch.nn.Parameter(p0[:n].double().clone())
    ref = torch.optim.Adam([q], lr=ADAM_LR)
    ref.state[q] = {"step": torch.tensor(0.0), "exp_avg": m0[:n].double().clone(), "exp_avg_sq": v0[:n].double().clone()}
    coef = float(torch.tensor(ADAM_COEF, dtype=torch.float32)) if "_clip" in entry else 1.0
    for _ in range(3):
        q.grad = g0[:n].double() * coef
        ref.step()
    p = _adam_run(lib, dev, entry, n, 3)[0]
    err = float((p[:n].double() - q.detach()).abs().max())
    print(f"{entry} n={n}: max |hip - float64| = {err:.3e}")
    assert err < 1e-5                           # the bound of test_clipped_flat_adam_against_..._in_float64


# ---------------------------------------------------------------- accumulating gather
class _TwoBranch(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.a, self.b = torch.nn.Linear(37, 19), torch.nn.Linear(37, 19)

    def forward(self, x, both=True):
        return self.a(x).tanh().sum() + (self.b(x).tanh().sum() if both else 0.0)


def test_accumulating_gather_equals_autograd_accumulation_bit_for_bit():
    dev = _dev()
    _lib()
    from ign_hip.ddp import FlatParamBucket
    net = _TwoBranch().to(dev)
    ref = copy.deepcopy(net)
    xs = torch.randn(2, 8, 37, device=dev)
    bucket = FlatParamBucket(net, 1)
    # second micro-batch: branch b takes no part, its parameters get no gradient
    for k, both in enumerate((True, False)):
        ref(xs[k], both).backward()                               # autograd accumulates into ref's p.grad
        net(xs[k], both).backward()
        bucket.gather(accumulate=k > 0)
        if k == 0:
            first = [v.clone() for v in bucket.views]
            bucket.zero_grad()
        assert all(p.grad is None for p in net.parameters())
    for (name, q), v, f in zip(ref.named_parameters(), bucket.views, first):
        assert torch.equal(v, q.grad), name
        if name.startswith("b."):
            assert torch.equal(v, f), name                        # no gradient in the second micro-step: the first value stays
        else:
            assert not torch.equal(v, f), name
    assert bucket._dirty == [True] * 4
    bucket.gather()                                               # what FlatAdam.step / allreduce do: closes the cycle, keeps the sums
    for (name, q), v, p in zip(ref.named_parameters(), bucket.views, net.parameters()):
        assert p.grad is v and torch.equal(v, q.grad), name


# ---------------------------------------------------------------- harness
ARGV = ["--model", "InterpGN", "--dnn_type", "FCN", "--data", "SYNTH", "--synthetic", "44,4,60,3", "--batch_size", "8", "--amp",
        "--train_epochs", "2", "--num_workers", "0", "--seed", "0", "--beta_schedule", "cosine", "--lr_decay", "--patience", "10",
        "--gradient_accumulation_steps", "2"]
# 44 samples at batch 8: five full batches and a ragged one of 4 per epoch = three optimizer steps per epoch; under --hipgraph the
# first micro-step and the first closing step of an epoch run eagerly and are captured, the next three batches are replays, the
# ragged closing step is eager; the second epoch has a new (beta, lr) key and captures again
OPT_STEPS = 6


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """mode -> (final state_dict on the host, grad_norm launches, gather_acc launches); each mode trained once"""
    done = {}

    def run_mode(mode):
        if mode in done:
            return done[mode]
        lib = _lib()
        import run
        from exp.experiment_classification import Experiment

        class TorchClipped(Experiment):
            """the same loop with nn.utils.clip_grad_norm_ and autograd's own accumulation"""

            def __init__(self, args):
                super().__init__(args)
                self._flat_step = False

        clip = "0" if mode == "eager_noclip" else "0.5"
        a = run.get_args(ARGV + ["--dataset", mode, "--gradient_clip", clip] + (["--hipgraph"] if mode == "graph" else []))
        a.min_epochs = 10                      # no early-stopping checkpoint: train() leaves the trained weights in place
        here = os.getcwd()
        os.chdir(tmp_path_factory.mktemp(mode))
        try:
            run.set_seed(0)
            e = (TorchClipped if mode == "torch" else Experiment)(a)
            assert e.device.type == "cuda"
            torch.manual_seed(123)
            timed = mode.startswith("eager")   # the event timers are not for use under capture
            if timed:
                lib.timing_enable(True)
            try:
                e.train()
                counts = (lib.timing_read("grad_norm")[1], lib.timing_read("gather_acc")[1]) if timed else (None, None)
            finally:
                if timed:
                    lib.timing_enable(False)
            if mode == "graph":
                assert e._graph_eligible(False) and set(e._graphed[1]) == {"micro", "close"} and e.optimizer.capturable
        finally:
            os.chdir(here)
        done[mode] = ({k: v.detach().cpu().clone() for k, v in e.model.state_dict().items()},) + counts
        return done[mode]

    return run_mode


def test_harness_clip_and_accumulation_equal_the_torch_clipped_trajectory(runs):
    _dev()
    new, ref = runs("eager")[0], runs("torch")[0]
    for k, v in new.items():
        w = ref[k].float()
        err, bound = float((v.float() - w).abs().max()), 2e-4 * max(1.0, float(w.abs().max()))
        print(f"{k}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound, k                 # the bound of test_harness_accumulation_and_clipping_on_the_flat_path


def test_hipgraph_clip_and_accumulation_is_bitwise_the_eager_run(runs):
    _dev()
    eager, graph = runs("eager")[0], runs("graph")[0]
    for k, v in eager.items():
        assert torch.equal(v, graph[k]), k


def test_grad_norm_fires_once_per_optimizer_step_and_never_without_clipping(runs):
    _dev()
    _, norms, accs = runs("eager")
    assert norms == OPT_STEPS and accs == OPT_STEPS             # one adding gather per cycle of two micro-steps
    _, norms, accs = runs("eager_noclip")
    assert norms == 0 and accs == OPT_STEPS
