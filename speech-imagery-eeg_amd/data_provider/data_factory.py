"""``data_provider(args, flag, bin_edges=None) -> (Dataset, DataLoader)`` -- the loader contract of
IGN/data_factory/data_factory.py:29-137 for the classification and regression tasks.

Batches are ``(X[B, T, C] float32, y[B, 1], mask[B, T] bool)``.  Registry keys follow the reference
(``UEA``, ``EEG``, ``EEG3``, ``Monash``); ``SYNTH`` is the synthetic benchmark provider.  Under ``torch.distributed`` each
rank iterates a disjoint, equally sized slice of a shared permutation (ign_hip.ddp.shard_indices).
"""
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader, Sampler

import functools

from data_provider.data_loader import Monashloader, UEAloader
from data_provider.eeg_npy import EEGNpyDataset, EEGNpyDataset3Class, collate_raw, collate_raw_group
from data_provider.synthetic import SyntheticEEG
from data_provider.uea import collate_fn, collate_subsampled

data_dict = {
    'UEA': UEAloader,
    'EEG': EEGNpyDataset,           # 39 classes
    'EEG3': EEGNpyDataset3Class,    # 3 classes
    'SYNTH': SyntheticEEG,
    'Monash': Monashloader,         # regression (float targets)
}


class RankShardSampler(Sampler):
    """Global permutation from a shared seed; rank r takes the r-th contiguous slice."""

    def __init__(self, n, rank, world, shuffle, seed=0):
        self.n, self.rank, self.world, self.shuffle, self.seed, self.epoch = n, rank, world, shuffle, seed, 0

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __iter__(self):
        from ign_hip.ddp import shard_indices
        self.epoch += 1
        return iter(shard_indices(self.n, self.rank, self.world, self.epoch, self.seed, self.shuffle).tolist())

    def __len__(self):
        return self.n // self.world


def data_provider(args, flag, bin_edges=None):
    flag = flag.lower()
    if args.task_name == 'regression':
        return _regression_provider(args, flag, bin_edges)
    if args.task_name != 'classification':
        raise NotImplementedError(f"task_name={args.task_name!r}: only the classification and regression paths are rebuilt "
                                  f"(SURVEY section 2 marks forecasting / anomaly out of scope)")
    if args.data not in data_dict:
        raise KeyError(f"--data {args.data!r} not in {sorted(data_dict)}")
    Data = data_dict[args.data]
    shuffle = flag != 'test'
    if args.data == 'SYNTH':
        shape = getattr(args, 'synthetic', None) or "8192,122,1000,3"
        n, C, T, N = (int(v) for v in shape.split(','))
        data_set = Data(flag=flag, n=n if flag == 'train' else max(args.batch_size, n // 8), seq_len=T, enc_in=C,
                        num_classes=N)
    elif args.data in ('EEG', 'EEG3'):
        # on a GPU the items stay RAW and the batch is standardised + transposed on the device (device_prefetch.py)
        raw = bool(getattr(args, 'device_standardise', torch.cuda.is_available()))
        # the --eeg_* flags as one chain; its "a rate equal to sfreq is no stage" line is the train split's to print
        from data_provider.eeg_chain import EEGChain
        data_set = Data(root_path=args.root_path, flag=flag, test_size=getattr(args, 'test_size', 0.2),
                        val_size=getattr(args, 'val_size', 0.1), raw=raw,
                        chain=EEGChain.from_args(args, notice=print if flag == 'train' else None))
    else:
        data_set = Data(root_path=args.root_path, flag=flag)

    max_len = getattr(data_set, 'seq_len', None) or getattr(args, 'seq_len', None)
    sampler = None
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 and flag == 'train':
        sampler = RankShardSampler(len(data_set), dist.get_rank(), dist.get_world_size(), shuffle,
                                   seed=max(0, getattr(args, 'seed', 0)))
    raw = bool(getattr(data_set, 'raw', False))
    stage = getattr(data_set, 'spatial', None)                          # an active --eeg_spatial: the raw batch carries its group ids
    if args.data == 'SYNTH' and args.num_workers == 0:
        # samples are rows of one in-memory tensor: a batch is one multi-threaded gather into a pinned buffer
        from data_provider.device_prefetch import TensorBatchLoader
        return data_set, TensorBatchLoader(data_set, args.batch_size, shuffle=shuffle, sampler=sampler,
                                           pin_memory=torch.cuda.is_available())
    loader = DataLoader(data_set, batch_size=args.batch_size, shuffle=(shuffle and sampler is None), sampler=sampler,
                        num_workers=args.num_workers, drop_last=False, pin_memory=torch.cuda.is_available(),
                        collate_fn=(collate_raw if stage is None else collate_raw_group) if raw
                        else (lambda b: collate_fn(b, max_len=max_len)))
    loader.eeg_chain = data_set.chain if raw else None              # raw items: Experiment._prefetch builds the device transform from it
    return data_set, loader


def ordered_loader(loader):
    """An unshuffled, un-sharded loader over the data set of `loader` (a DataLoader, a TensorBatchLoader, or a DevicePrefetcher
    around either): batch i holds the data set's items i*batch_size ..., on every rank, so a sample's ordinal in the stream is
    its data set index -- what a pass that reports sample indices needs (utils/shapelet_project.py).  Same batch size, collate_fn
    and eeg_chain attribute; no sampler, drop_last=False.  A DataLoader draws its per-iteration seed
    from a generator of its own, so iterating the result leaves torch's global RNG stream where it was."""
    from data_provider.device_prefetch import DevicePrefetcher, TensorBatchLoader
    if isinstance(loader, DevicePrefetcher):
        return DevicePrefetcher(ordered_loader(loader.loader), loader.device, transform=loader.transform, depth=loader.depth)
    if isinstance(loader, TensorBatchLoader):
        out = TensorBatchLoader(loader.dataset, loader.batch_size, shuffle=False, sampler=None, pin_memory=loader.pin)
    elif isinstance(loader, DataLoader):
        out = DataLoader(loader.dataset, batch_size=loader.batch_size, shuffle=False, sampler=None, num_workers=loader.num_workers,
                         drop_last=False, pin_memory=loader.pin_memory, collate_fn=loader.collate_fn, generator=torch.Generator())
    else:
        raise TypeError(f"ordered_loader: expected a DataLoader, TensorBatchLoader or DevicePrefetcher, got {type(loader).__name__}")
    out.eeg_chain = getattr(loader, 'eeg_chain', None)
    return out


def _regression_provider(args, flag, bin_edges):
    """IGN/data_factory/data_factory.py:123-137.  `bin_edges`: None for the train split (the loader derives them), the train
    split's edges for val / test.  Every batch is padded / clipped to the dataset's max_seq_len and subsampled with the
    dataset's one stride (repair R2: the reference clips later batches to the first batch's subsampled length).  --batch_size
    also for test (the reference evaluates one series at a time; eval-mode outputs do not depend on the batch here)."""
    if args.data != 'Monash':
        raise KeyError(f"--data {args.data!r}: the regression task reads the Monash archive (--data Monash)")
    data_set = Monashloader(root_path=args.root_path, flag=flag, bin_edges=bin_edges)
    sampler = None
    shuffle = flag == 'train'
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 and flag == 'train':
        sampler = RankShardSampler(len(data_set), dist.get_rank(), dist.get_world_size(), shuffle,
                                   seed=max(0, getattr(args, 'seed', 0)))
    loader = DataLoader(data_set, batch_size=args.batch_size, shuffle=(shuffle and sampler is None), sampler=sampler,
                        num_workers=args.num_workers, drop_last=False, pin_memory=torch.cuda.is_available(),
                        collate_fn=functools.partial(collate_subsampled, max_len=data_set.max_seq_len, stride=data_set.stride))
    return data_set, loader
