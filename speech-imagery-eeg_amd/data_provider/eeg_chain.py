"""The EEG front end as ONE ordered chain, from the flags to the prefetch stream (``--data EEG`` / ``EEG3``):

    artifact -> spatial -> iir -> resample -> preprocess (-> standardise: always last, inside the preprocess stage when there is one)

``EEGChain`` is the parsed form (the five specs, ``--target_channels`` / ``--target_timepoints``, the cross-flag rules in ``check``),
``EEGChain.resolve`` gives the resolved form, ``ResolvedChain``: the ACTIVE stages only, in that order.  A stage is the object that owns
its data (``ResolvedArtifact``, ``SpatialStage``, ``ResolvedIIR``, ``ResolvedResample``, ``Resolved`` / ``ResolvedBank``), with a ``name`` and four methods:

    out_shape(C, T) -> (C, T)      the shape that leaves the stage for the one that enters
    apply_item(x (C,T), group)     the numpy rule of the CPU item path; the preprocess stage returns (Tv, C) standardised
    device_fn(device)              uploads the stage's table once -> ``x (B,C,T), gid -> x``, one launch; preprocess: ``-> (X[B,T,C], mask)``
    save(directory)                writes the stage's record file -> its path (None: the stage keeps no record)

The order exists here and nowhere else.  Batch contract of the transform: ``(X[B,C,T] raw, y, gid[B] or None) -> (X[B,T,C], y, mask[B,T])``.
"""
import os

import numpy as np
import torch

from data_provider.device_prefetch import standardise_raw_batch
from utils.eeg_artifact import parse_eeg_artifact, resolve_artifact
from utils.eeg_filter import parse_eeg_preprocess, resolve
from utils.eeg_iir import iir_numpy, parse_eeg_iir, resolve_iir
from utils.eeg_resample import parse_eeg_resample, resolve_resample, same_rate
from utils.eeg_spatial import SpatialStage, compose, load_matrix, needs_groups, parse_eeg_spatial

ORDER = ('artifact', 'spatial', 'iir', 'resample', 'preprocess')
_ACTS_ON = dict(preprocess="filters the raw CHISCO shards", spatial="acts on the electrodes of the raw CHISCO shards",
                iir="filters the rows of the raw CHISCO shards", resample="resamples the rows of the raw CHISCO shards",
                artifact="judges the rows of the raw CHISCO shards")


def _resolve_spatial(spec, Cin, root_path, n, notice):
    """--eeg_spatial: compose W0, and -- when the stage needs groups (an alignment, or one matrix per group) -- read the optional
    <root>/subject.npy (n,) and map its ids to dense 0..G-1 over the WHOLE file, sorted by id, before the split: every split sees
    the same mapping.  -> (SpatialStage, group (n,) int32)."""
    matrix = load_matrix(spec)
    W0 = compose(spec, Cin, matrix)
    group, groups, labels = np.zeros(n, dtype=np.int32), 1, None
    if needs_groups(spec, matrix):
        sp = os.path.join(root_path, "subject.npy")
        if os.path.exists(sp):
            ids = np.load(sp, allow_pickle=False)
            if ids.shape != (n,) or not np.issubdtype(ids.dtype, np.integer):
                raise ValueError(f"{sp}: expected {n} integer subject ids, got {ids.dtype} {ids.shape}")
            labels, dense = np.unique(ids, return_inverse=True)
            group, groups = dense.astype(np.int32).reshape(n), int(len(labels))
        elif notice is not None:
            notice(f"eeg_spatial: {sp} not found; all {n} trials are one group")
    if W0.shape[0] > 1 and W0.shape[0] != groups:
        raise ValueError(f"--eeg_spatial: the matrix holds {W0.shape[0]} groups, the shards {groups}")
    return SpatialStage(spec, W0, groups, labels), group


class EEGChain:
    """The parsed form.  Flag texts (or specs already parsed) by keyword; `notice` hears the resampler's "a rate equal to sfreq is
    no stage" line.  The flags are parsed in the order the driver has always reported a malformed one in; --eeg_artifact, the
    youngest, last."""

    def __init__(self, spatial=None, iir=None, resample=None, preprocess=None, target_channels=None, target_timepoints=None, notice=None,
                 artifact=None):
        self.preprocess = parse_eeg_preprocess(preprocess)
        self.spatial = parse_eeg_spatial(spatial)
        self.iir = parse_eeg_iir(iir)
        self.resample = parse_eeg_resample(resample, notice=notice)
        self.target_channels, self.target_timepoints = target_channels, target_timepoints
        self.artifact = parse_eeg_artifact(artifact)

    @classmethod
    def from_args(cls, args, notice=None):
        return cls(*(getattr(args, 'eeg_' + name, None) for name in ('spatial', 'iir', 'resample', 'preprocess')),
                   getattr(args, 'target_channels', None), getattr(args, 'target_timepoints', None), notice,
                   artifact=getattr(args, 'eeg_artifact', None))

    active = property(lambda self: [name for name in ORDER if getattr(self, name).active], doc="the active stages' names, in ORDER")

    def check(self, data_name):
        """The cross-flag rules: every active stage needs the raw CHISCO shards, and neighbours along the chain agree on the rate."""
        for name in ('preprocess', 'spatial', 'iir', 'resample', 'artifact'):
            if getattr(self, name).active and data_name not in ('EEG', 'EEG3'):
                raise ValueError(f"--eeg_{name} {_ACTS_ON[name]} (--data EEG / EEG3), not --data {data_name}")
        # one walk along the chain with the current rate carried forward.  A rate that a flag names is compared as written; behind
        # the resampler the rate is a rounded quotient and is compared with same_rate (as is the resampler's own sfreq).
        iir, rs, pre = self.iir, self.resample, self.preprocess
        rate, quotient = (iir.sfreq, False) if iir.active else (None, False)
        if rs.active:
            if rate is not None and not same_rate(rate, rs.sfreq):
                raise ValueError(f"--eeg_resample: the rows arrive at sfreq={rs.sfreq:g} Hz, but --eeg_iir names sfreq={rate:g} Hz")
            rate, quotient = rs.rate, True
        if pre.active and rate is not None:
            if quotient and not same_rate(pre.sfreq, rate):
                raise ValueError(f"--eeg_resample: the rows leave at {rate:g} Hz, but --eeg_preprocess names sfreq={pre.sfreq:g} Hz")
            if not quotient and pre.sfreq != rate:
                raise ValueError(f"--eeg_iir: sfreq={rate:g} Hz, but --eeg_preprocess names sfreq={pre.sfreq:g} Hz")

    def resolve(self, Cin, Tin, root_path, n, notice=None):
        """Against raw items (Cin, Tin) of the n trials under `root_path` -> ResolvedChain.  `notice`: print for the train split."""
        C, T, stages, group = int(Cin), int(Tin), [], None
        for name in self.active:
            if name == 'artifact':
                stage = resolve_artifact(self.artifact, C, T)
            elif name == 'spatial':
                stage, group = _resolve_spatial(self.spatial, C, root_path, n, notice)
            elif name == 'iir':
                stage = resolve_iir(self.iir, T)
            elif name == 'resample':
                stage = resolve_resample(self.resample, T)
            else:
                stage = resolve(self.preprocess, C, T, self.target_channels, self.target_timepoints, notice=notice)
            stages.append(stage)
            C, T = stages[-1].out_shape(C, T)           # what the next stage, and at the end the models, are built for
        return ResolvedChain(stages, (C, T), group)


class ResolvedChain:
    """The resolved form: `stages` (the active ones, in ORDER), `shape` = (enc_in, seq_len) of what the models see, `group` (n,)
    int32 under an active spatial stage (else None)."""

    def __init__(self, stages, shape, group=None):
        self.stages, self.shape, self.group = list(stages), tuple(shape), group

    names = property(lambda self: [s.name for s in self.stages])

    def stage(self, name):
        """stage `name`; None when it is not active"""
        return next((s for s in self.stages if s.name == name), None)

    def device_transform(self, device):
        """The prefetcher's transform, built once per loader: every table goes to `device` here and the spatial matrices are read here
        -- so build it after the alignment is fitted.  One launch per stage and batch, then the tail: the preprocess stage's filter
        bank (it standardises and returns the mask), else standardise_raw_batch -- with no stage at all the transform itself."""
        if not self.stages:
            return standardise_raw_batch
        fns = [s.device_fn(device) for s in self.stages]
        tail = fns.pop() if self.stages[-1].name == 'preprocess' else None

        def transform(batch):
            x, y, gid = batch
            for fn in fns:
                x = fn(x, gid)
            if tail is None:
                return standardise_raw_batch((x, y, None))
            xs, mask = tail(x, gid)
            return xs, y, mask
        return transform

    def alignment_post(self, device):
        """fit_alignment's `post`: the IIR stage alone (never the resampler), None without one.  A tensor on the GPU `device` goes through
        the stage's device function, a host array through the float64 rule unrounded: the alignment is fitted on what the model will see."""
        iir = self.stage('iir')
        if iir is None:
            return None
        run = iir.device_fn(device) if torch.device(device).type == 'cuda' else None

        def post(y):
            if torch.is_tensor(y) and y.is_cuda:
                return run(y, None)
            return iir_numpy(y.numpy() if torch.is_tensor(y) else y, iir.table, iir.pad, iir.g0)
        return post

    def save(self, directory):
        """the record files of the active stages, beside the checkpoint -> their paths"""
        return [p for p in (s.save(directory) for s in self.stages) if p is not None]
