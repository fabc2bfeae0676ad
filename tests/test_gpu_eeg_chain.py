"""The EEG front end as one chain on the device: with all four flags on and the Euclidean alignment fitted, what Experiment._prefetch
yields is ops.eeg_spatial -> ops.eeg_iir -> ops.eeg_resample -> ops.eeg_filterbank composed by hand per batch, bit for bit, with one
launch per stage and batch; with the flags at their defaults none of the three stage kernels runs.  Shards: 6 electrodes, 3
subjects, T = 400, batches of 8."""
from argparse import Namespace
from types import SimpleNamespace

import pytest
import torch

from eeg_spatial_cases import write_shards

pytestmark = pytest.mark.gpu
STAGES = ("eeg_spatial", "eeg_iir", "eeg_resample")
ALL_ON = dict(eeg_spatial="ref=car,align=euclid", eeg_iir="hp=1,notch=50", eeg_resample="rate=256", eeg_preprocess="band=8:30,sfreq=256")


def _experiment(root, dev, **flags):
    """the part of Experiment that loads the three splits and fits the alignment, without a model"""
    import speech_imagery_eeg_amd  # noqa: F401
    from exp.experiment_classification import Experiment
    args = Namespace(task_name="classification", data="EEG", root_path=str(root), batch_size=8, num_workers=0, seed=0,
                     device_standardise=True, **flags)
    me = SimpleNamespace(args=args, device=dev, rank=0)
    me._fit_eeg_spatial = lambda: Experiment._fit_eeg_spatial(me)
    Experiment._load_data(me)
    return me, Experiment


def _batches(me, Experiment, loader):
    """(the loader's raw batches, the same batches through Experiment._prefetch): one seed, so one order"""
    torch.manual_seed(11)
    raw = [tuple(None if t is None else t.clone() for t in b) for b in loader]
    torch.manual_seed(11)
    return raw, list(Experiment._prefetch(me, loader))


def test_prefetch_is_the_four_ops_composed_by_hand_with_one_launch_per_stage_and_batch(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    dev = torch.device("cuda:0")
    write_shards(str(tmp_path), T=400)
    me, Experiment = _experiment(tmp_path, dev, **ALL_ON)
    from ign_hip import _lib, ops
    assert all(d.spatial.fitted and d.spatial.W.shape == (3, 6, 6) for d in (me.train_data, me.val_data, me.test_data))
    assert me.train_data.spatial.W.tobytes() == me.test_data.spatial.W.tobytes()
    _lib.timing_enable(True)                                            # behind the fit: its launches are not the prefetcher's
    try:
        for flag in ("train", "test"):
            ds, loader = (me.train_data, me.train_loader) if flag == "train" else (me.test_data, me.test_loader)
            assert loader.eeg_chain is ds.chain and ds.chain.names == ["spatial", "iir", "resample", "preprocess"]
            assert (ds.enc_in, ds.seq_len, ds.iir.pad, ds.resample.Tout, len(ds.pre.taps)) == (6, 205, 21, 205, 107)
            before = [_lib.timing_read(name)[1] for name in STAGES]     # the hand composition below launches the same kernels
            raw, got = _batches(me, Experiment, loader)
            torch.cuda.synchronize()
            assert len(got) == len(raw) == -(-len(ds) // 8)
            assert [_lib.timing_read(name)[1] - n for name, n in zip(STAGES, before)] == [len(raw)] * 3, flag
            W = torch.from_numpy(ds.spatial.W).to(dev)
            coef, tab = torch.from_numpy(ds.iir.table).to(dev), torch.from_numpy(ds.resample.tab).to(dev)
            p = ds.pre
            taps = torch.as_tensor(p.taps2d, dtype=torch.float32).to(dev)
            for (X, yb, mask), (x, y, gid) in zip(got, raw):
                assert gid.dtype == torch.int32 and len(set(gid.tolist())) > 1
                v = ops.eeg_spatial(x.to(dev), W, gid.to(dev))
                v = ops.eeg_iir(v, coef, pad=ds.iir.pad, g0=ds.iir.g0)
                v = ops.eeg_resample(v, tab, up=64, down=125, half_len=ds.resample.hl, edge="reflect")
                want, want_mask = ops.eeg_filterbank(v, taps, None, decimate=p.q, edge=p.edge, channels=p.Cout, timepoints=p.Tout)
                assert X.is_cuda and tuple(X.shape) == (x.shape[0], 205, 6) and bool(torch.isfinite(X).all())
                assert torch.equal(X, want) and torch.equal(mask, want_mask) and torch.equal(yb.cpu(), y)
    finally:
        _lib.timing_enable(False)


def test_default_flags_launch_none_of_the_three_stage_kernels(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    dev = torch.device("cuda:0")
    write_shards(str(tmp_path), T=400)
    from data_provider import device_prefetch
    me, Experiment = _experiment(tmp_path, dev)
    from ign_hip import _lib
    _lib.timing_enable(True)
    try:
        for loader in (me.train_loader, me.test_loader):
            assert loader.eeg_chain.stages == []
            pf = Experiment._prefetch(me, loader)
            assert pf.transform is device_prefetch.standardise_raw_batch
            got = list(pf)
            assert got and all(tuple(X.shape[1:]) == (400, 6) and bool(m.all()) for X, _, m in got)
        torch.cuda.synchronize()
        for name in STAGES:
            assert _lib.timing_read(name)[1] == 0, name
    finally:
        _lib.timing_enable(False)
