"""Host -> device double buffering for the training loop.

Once the step runs in ~14 ms the synchronous ``.to(device)`` of IGN/exp/experiment_classification.py:315-317 and the
per-item CPU normalisation in the DataLoader workers become the bottleneck (a 256-sample CHISCO batch is 125 MB: ~2 ms
over PCIe Gen5, and ~0.5 ms of CPU z-scoring per sample).  ``DevicePrefetcher`` wraps any DataLoader of the batch contract
``(X, y, mask)``: batch i+1 is pinned and copied on a side HIP stream while batch i trains; an optional ``transform`` runs
on that stream too -- for the CHISCO shards the loader ships RAW (B,C,T) microvolt tensors and the per-sample
standardisation + transpose happen on the GPU (``ops.standardise_nct_to_btc``; with ``--eeg_preprocess`` the filter, decimation
and fitting in front of it too: ``ops.eeg_filterbank``, a one-band spec as the bank of one).  On a CPU device it is a pass-through.
"""
import torch


def standardise_raw_batch(batch):
    """transform for loaders that yield raw (X[B,C,T], y, None): -> (X[B,T,C] standardised, y, mask ones[B,T])."""
    from ign_hip import ops
    x, y, _ = batch
    xs = ops.standardise_nct_to_btc(x.float())
    return xs, y, torch.ones(xs.shape[0], xs.shape[1], device=xs.device, dtype=torch.bool)


def preprocess_raw_batch(pre, device):
    """transform for raw loaders under --eeg_preprocess, built once per loader: `pre` is the data set's resolved spec
    (utils.eeg_filter.Resolved or ResolvedBank; one band is the bank of one); its taps go to the device here, once.
    (X[B,Cin,Tin], y, None) -> (X[B,Tout,nb*Cout] filtered, decimated, fitted and standardised, band-major, y,
    mask[B,Tout] = t < Tv)."""
    from ign_hip import ops
    taps = torch.as_tensor(pre.taps2d, dtype=torch.float32).to(device)
    quad = None if pre.quad is None else torch.as_tensor(pre.quad, dtype=torch.float32).to(device)
    kw = dict(decimate=pre.q, edge=pre.edge, channels=pre.Cout, timepoints=pre.Tout)

    def transform(batch):
        x, y, _ = batch
        xs, mask = ops.eeg_filterbank(x.float(), taps, quad, **kw)
        return xs, y, mask
    return transform


def spatial_raw_batch(W, inner):
    """transform for raw loaders under --eeg_spatial: `W` (G,Cs,Cin) float32 on the device, `inner` the transform that would run
    without the stage (standardise_raw_batch, or preprocess_raw_batch's).  (X[B,Cin,T], y, gid[B] int32) -> inner on
    (W[gid[b]] . X[b] (B,Cs,T), y, None): one more launch on the prefetch stream, in front of the others."""
    from ign_hip import ops
    one_group = W.shape[0] == 1

    def transform(batch):
        x, y, gid = batch
        return inner((ops.eeg_spatial(x.float(), W, None if one_group else gid), y, None))
    return transform


def iir_stage_fn(stage):
    """x (B,C,T) on the GPU -> ops.eeg_iir(x) for a resolved --eeg_iir stage (utils.eeg_iir.ResolvedIIR); the float64 section table
    is uploaded once, with the first batch, as the FIR taps are once per loader."""
    from ign_hip import ops
    coef = {}

    def run(x):
        if x.device not in coef:
            coef[x.device] = torch.from_numpy(stage.table).to(x.device)
        return ops.eeg_iir(x.float(), coef[x.device], pad=stage.pad, g0=stage.g0)
    return run


def iir_post(stage):
    """The stage as utils.eeg_spatial.fit_alignment's `post`: a GPU tensor goes through ops.eeg_iir, a host array through the float64
    rule unrounded -- so the alignment is fitted on what the model will see."""
    from utils.eeg_iir import iir_numpy
    run = iir_stage_fn(stage)

    def post(y):
        if torch.is_tensor(y) and y.is_cuda:
            return run(y)
        return iir_numpy(y.numpy() if torch.is_tensor(y) else y, stage.table, stage.pad, stage.g0)
    return post


def iir_raw_batch(stage, inner):
    """transform for raw loaders under --eeg_iir: `stage` the resolved sections, `inner` the transform that would run without the
    stage (standardise_raw_batch, or preprocess_raw_batch's).  (X[B,C,T], y, third) -> inner on (the rows filtered forward and
    backward along time (B,C,T), y, third): one more launch on the prefetch stream, behind the spatial stage (spatial_raw_batch wraps
    this one) and in front of the others."""
    run = iir_stage_fn(stage)

    def transform(batch):
        x, y, third = batch
        return inner((run(x), y, third))
    return transform


def resample_raw_batch(stage, inner):
    """transform for raw loaders under --eeg_resample: `stage` the resolved ratio (utils.eeg_resample.ResolvedResample), `inner` the
    transform that would run without the stage.  (X[B,C,Tin], y, third) -> inner on (the rows resampled to Tout samples (B,C,Tout), y,
    third): one more launch on the prefetch stream, behind the IIR stage (iir_raw_batch wraps this one) and in front of the others.
    The fp32 phase table is uploaded once, with the first batch."""
    from ign_hip import ops
    tab = {}

    def transform(batch):
        x, y, third = batch
        if x.device not in tab:
            tab[x.device] = torch.from_numpy(stage.tab).to(x.device)
        x = ops.eeg_resample(x.float(), tab[x.device], up=stage.up, down=stage.down, half_len=stage.hl, edge=stage.edge)
        return inner((x, y, third))
    return transform


class DevicePrefetcher:
    def __init__(self, loader, device, transform=None, depth=2):
        self.loader, self.device, self.transform, self.depth = loader, torch.device(device), transform, max(1, depth)
        self.dataset = getattr(loader, "dataset", None)

    def __len__(self):
        return len(self.loader)

    def _stage(self, batch, stream):
        def put(t):
            if not torch.is_tensor(t):
                return t
            if not t.is_pinned():
                t = t.pin_memory()
            return t.to(self.device, non_blocking=True)
        with torch.cuda.stream(stream):
            out = tuple(put(t) for t in batch)
            if self.transform is not None:
                out = self.transform(out)
            ev = torch.cuda.Event()
            ev.record(stream)
        return out, ev

    def __iter__(self):
        if self.device.type != "cuda":
            for batch in self.loader:
                yield self.transform(batch) if self.transform is not None else batch
            return
        stream = torch.cuda.Stream(self.device)
        queue = []
        it = iter(self.loader)
        done = False
        while True:
            while not done and len(queue) < self.depth:
                try:
                    queue.append(self._stage(next(it), stream))
                except StopIteration:
                    done = True
            if not queue:
                return
            out, ev = queue.pop(0)
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            for t in out:
                if torch.is_tensor(t):
                    t.record_stream(cur)        # allocated on the copy stream, consumed on the compute stream
            yield out


class TensorBatchLoader:
    """DataLoader stand-in for a data set whose samples are the rows of ONE in-memory tensor (``dataset.x`` (n, T, C) float32,
    ``dataset.y`` (n,)): the synthetic benchmark provider, and any fixed-length set after it has been read.

    A ``DataLoader`` fetches 256 items, stacks them (one 125 MB copy on one thread) and, with ``pin_memory``, copies the batch a
    second time -- at the CHISCO shape that is more host time than the 12 ms the step takes on the GPU.  Here a batch is ONE
    multi-threaded ``index_select`` straight into a pinned buffer (the caching host allocator hands the block back once the
    asynchronous copy that read it has completed), so the DevicePrefetcher's ``.to(device, non_blocking=True)`` is the only other
    copy.  Same batch contract as ``collate_fn`` (IGN/data_factory/uea.py:7-42): ``(X[B,T,C] float32, y[B,1], mask[B,T] bool)``;
    same iteration semantics as the DataLoader it replaces (fresh permutation per epoch from torch's global generator, a
    ``sampler`` yielding indices is honoured, ``drop_last=False``)."""

    def __init__(self, dataset, batch_size, shuffle=False, sampler=None, pin_memory=True):
        self.dataset, self.batch_size, self.shuffle, self.sampler = dataset, int(batch_size), bool(shuffle), sampler
        self.pin = bool(pin_memory) and torch.cuda.is_available()
        self.device_transform = None

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.dataset)
        return (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        ds = self.dataset
        if self.sampler is not None:
            order = torch.as_tensor(list(iter(self.sampler)), dtype=torch.int64)
        elif self.shuffle:
            order = torch.randperm(len(ds))
        else:
            order = torch.arange(len(ds))
        T, C = ds.x.shape[1], ds.x.shape[2]
        for i in range(0, order.numel(), self.batch_size):
            idx = order[i:i + self.batch_size]
            k = idx.numel()
            X = torch.empty(k, T, C, dtype=torch.float32, pin_memory=self.pin)
            torch.index_select(ds.x, 0, idx, out=X)
            y = ds.y.index_select(0, idx).unsqueeze(1).to(torch.int8)
            yield X, y, torch.ones(k, T, dtype=torch.bool)
