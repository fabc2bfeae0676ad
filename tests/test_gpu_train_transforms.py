"""The chain of the training-batch transforms (utils/train_transforms.py) on the GPU with all three flags on: its output is
mix_reference(augment_reference(warp_reference(x))) bit for bit under the one step seed, the soft labels are the draws', and an
all-ones mask gives what no lengths give.  One small ragged batch -- lengths 0 and 1 (nothing to warp, nothing to shift), a full row
and three in between -- at C = 4 (the vector paths), C = 3 (the element and seam paths) and T * C = 141 (a partial tail quad).  Noise
is off, so every reference is bitwise.  The single ops have their own tests (test_gpu_warp.py, test_gpu_augment.py, test_gpu_mix.py)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SENTINEL = 777.0
FLAGS = dict(warp="twarp=0.2,mwarp=0.1,wwarp=0.2", augment="shift=0.2,scale=0.1,chan_drop=0.2,time_mask=0.2", mix="mixup=0.4,cutmix=1")
B, STEP = 6, 3
SHAPES = [(48, 4), (48, 3), (47, 3)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import speech_imagery_eeg_amd  # noqa: F401
    return torch.device("cuda:0")


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("T,C", SHAPES, ids=[f"{B}x{t}x{c}" for t, c in SHAPES])
def test_chain_equals_the_three_references_composed_bit_for_bit(T, C):
    dev = _dev()
    from ign_hip import ops
    from utils.augment import augment_reference, step_seed
    from utils.mix import mix_draws, mix_reference
    from utils.train_transforms import TrainTransforms
    from utils.warp import warp_reference
    chain = TrainTransforms.from_args(Namespace(seed=0, **FLAGS), rank=0)
    assert chain and chain.base == 0 and None not in (chain.warp, chain.augment, chain.mix)
    lens = [T, 1, 0, 17, 30, 5]
    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(5))
    mask = torch.zeros(B, T)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
        x[b, n:] = SENTINEL
    label = torch.arange(B) % 3
    xd = x.to(dev)
    out, (label_b, lam) = chain(xd, label.to(dev), mask.to(dev), STEP)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x)                                  # the input is left as it was

    seed = step_seed(0, 0, STEP)
    roll, lam_h, span_h = mix_draws(seed, B, np.asarray(lens), chain.mix)
    want = warp_reference(x.numpy(), seed, lens, **chain.warp._asdict())
    want = augment_reference(want, seed, lens, **chain.augment._asdict())
    want = mix_reference(want, lens, roll, lam_h, span_h)
    assert _same_bits(out.cpu().numpy(), want)
    assert torch.equal(label_b.cpu(), label.roll(-roll)) and torch.equal(lam.cpu(), torch.from_numpy(lam_h))
    assert not np.array_equal(want[0], x[0].numpy())                 # the case exercises something
    assert np.array_equal(want[2], x[2].numpy())                     # n = 0: the row is its padding
    for b, n in enumerate(lens):
        assert bool((out[b, n:] == SENTINEL).all())

    # an all-ones mask gives what lengths = None gives
    full, (label_f, lam_f) = chain(xd, label.to(dev), torch.ones(B, T, device=dev), STEP)
    roll_f, lam_fh, span_fh = mix_draws(seed, B, T, chain.mix)
    plain = ops.augment(ops.warp(xd, seed, **chain.warp._asdict()), seed, **chain.augment._asdict())
    plain = ops.mix(plain, torch.from_numpy(lam_fh).to(dev), roll_f, span=torch.from_numpy(span_fh).to(dev))
    assert torch.equal(full, plain) and torch.equal(lam_f.cpu(), torch.from_numpy(lam_fh))
    assert torch.equal(label_f.cpu(), label.roll(-roll_f))
