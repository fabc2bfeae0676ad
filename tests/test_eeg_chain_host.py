"""The EEG front end as one chain (data_provider/eeg_chain.py), without a device: the fixed order spatial -> iir -> resample ->
preprocess for all 16 on/off combinations of the four flags, the CPU item path against the per-stage numpy rules composed by hand
(bytes), the cross-flag rules through the chain, the driver and the data set (the same strings), the device transform with the five
ops replaced by recorders, and the record files.  Shards: 6 electrodes, 3 subjects, T = 400 -- the IIR pad of 21, the 64/125
resampler and a 107-tap band all fit."""
import itertools
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from eeg_spatial_cases import write_shards

ORDER = ("spatial", "iir", "resample", "preprocess")
COMBOS = list(itertools.product((False, True), repeat=4))
RECORDS = dict(spatial="eeg_spatial.npz", iir="eeg_iir.json", resample="eeg_resample.json")


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    import speech_imagery_eeg_amd  # noqa: F401
    root = tmp_path_factory.mktemp("chain")
    X, _, subj = write_shards(str(root), T=400)
    M = np.random.RandomState(0).randn(3, 5, 6)                       # one 5 x 6 montage per subject: enc_in becomes 5
    np.save(root / "m.npy", M)
    return Namespace(root=root, X=X, M=M, dense=np.searchsorted(np.unique(subj), subj))


def _flags(shards, on):
    """the four flag texts of one combination; --eeg_preprocess names the rate it sees"""
    sp, iir, rs, pre = on
    return dict(eeg_spatial=f"ref=car,matrix={shards.root / 'm.npy'}" if sp else "none", eeg_iir="hp=1,notch=50" if iir else "none",
                eeg_resample="rate=256" if rs else "none",
                eeg_preprocess=("band=8:30,sfreq=256" if rs else "band=8:30") if pre else "none")


def _names(on):
    return [n for n, v in zip(ORDER, on) if v]


def _ns(shards, raw, **kw):
    return Namespace(task_name="classification", data="EEG", root_path=str(shards.root), batch_size=8, num_workers=0, seed=0,
                     device_standardise=raw, **kw)


@pytest.mark.parametrize("on", COMBOS, ids=lambda on: "+".join(_names(on)) or "none")
def test_order_is_fixed_however_the_namespace_was_filled(shards, on):
    from data_provider.eeg_chain import EEGChain
    flags = _flags(shards, on)
    for keys in (sorted(flags), sorted(flags, reverse=True), ["eeg_resample", "eeg_spatial", "eeg_preprocess", "eeg_iir"]):
        args = Namespace()
        for k in keys:
            setattr(args, k, flags[k])
        chain = EEGChain.from_args(args)
        assert chain.active == _names(on)
        chain.check("EEG")
        assert chain.resolve(6, 400, str(shards.root), 24).names == _names(on)


@pytest.mark.parametrize("on", COMBOS, ids=lambda on: "+".join(_names(on)) or "none")
def test_item_is_the_numpy_rules_composed_by_hand_and_the_shapes_fold(shards, on):
    from data_provider.data_factory import data_provider
    from data_provider.eeg_npy import per_sample_standardise
    from utils.eeg_filter import filterbank_numpy
    from utils.eeg_iir import iir_numpy
    from utils.eeg_resample import resample_numpy
    from utils.eeg_spatial import compose, spatial_numpy
    sp, iir, rs, pre = on
    ds, loader = data_provider(_ns(shards, False, **_flags(shards, on)), "train")
    assert loader.eeg_chain is None and ds.chain.names == _names(on)
    assert [ds.spatial is not None, ds.iir is not None, ds.resample is not None, ds.pre is not None] == list(on)
    assert all(a is b for a, b in zip(ds.chain.stages, [s for s in (ds.spatial, ds.iir, ds.resample, ds.pre) if s is not None]))
    assert (ds.enc_in, ds.seq_len) == ds.chain.shape == (5 if sp else 6, 205 if rs else 400)
    if pre:
        assert len(ds.pre.taps) == (107 if rs else 207)
    W0 = compose("ref=car", 6, shards.M)
    for i in (0, 5):
        j = ds.idx[i]
        v = shards.X[j]
        if sp:
            v = spatial_numpy(v, W0[shards.dense[j]].astype(np.float32), dtype=np.float32)
        if iir:
            assert ds.iir.pad == 21
            v = iir_numpy(v, ds.iir.table, 21, ds.iir.g0).astype(np.float32)
        if rs:
            v = resample_numpy(v, ds.resample.tab, 64, 125, ds.resample.hl, "reflect").astype(np.float32)
        if pre:
            p = ds.pre
            want = filterbank_numpy(v, p.taps2d.astype(np.float32), None, p.q, p.edge, p.Cout, p.Tout).astype(np.float32)
        else:
            want = per_sample_standardise(v).T
        got = ds[i][0].numpy()
        assert got.shape == (ds.seq_len, ds.enc_in) and got.dtype == np.float32 and got.tobytes() == want.tobytes()


# (--eeg_iir, --eeg_resample, --eeg_preprocess) -> the message, None where the three agree.  Every arm of the rate rules: a rate that a
# flag names is compared as written (iir against preprocess, `!=`), a rate behind the resampler -- and the resampler's own sfreq --
# within 1e-9 of each other (same_rate).  250.0000000001 Hz against 250 Hz shows the difference: refused without a resampler between
# the two flags, accepted with one.
A = "--eeg_resample: the rows arrive at sfreq={} Hz, but --eeg_iir names sfreq={} Hz"
B = "--eeg_resample: the rows leave at {} Hz, but --eeg_preprocess names sfreq={} Hz"
C = "--eeg_iir: sfreq={} Hz, but --eeg_preprocess names sfreq={} Hz"
RATES = [
    ("hp=1", "none", "none", None),
    ("none", "rate=256", "none", None),
    ("none", "none", "band=8:30", None),
    ("hp=1", "none", "band=8:30", None),
    ("hp=1,sfreq=250", "none", "band=8:30,sfreq=250", None),
    ("hp=1", "none", "band=8:30,sfreq=250", C.format(500, 250)),
    ("hp=1,sfreq=250", "none", "band=8:30", C.format(250, 500)),
    ("hp=1,sfreq=250.0000000001", "none", "band=8:30,sfreq=250", C.format(250, 250)),                 # `!=`: as written
    ("hp=1,sfreq=250.0000000001", "rate=128,sfreq=250", "band=8:30,sfreq=128", None),               # same_rate: a resampler between
    ("hp=1,sfreq=250.0000000001", "rate=128,sfreq=250", "none", None),
    ("hp=1", "rate=256", "band=8:30,sfreq=256", None),
    ("hp=1", "ratio=64/125", "band=8:30,sfreq=256", None),
    ("none", "ratio=1/3", "band=8:30,sfreq=166.6666666667", None),                                  # same_rate: a rounded quotient
    ("none", "ratio=1/3", "band=8:30,sfreq=166.67", B.format("166.667", "166.67")),
    ("hp=1,sfreq=250", "rate=256", "none", A.format(500, 250)),
    ("hp=1,sfreq=250", "rate=256", "band=8:30", A.format(500, 250)),                                # the first disagreement along the chain
    ("hp=1", "rate=256", "band=8:30", B.format(256, 500)),
    ("none", "rate=256", "band=8:30", B.format(256, 500)),
    ("none", "rate=256", "band=8:30,sfreq=250", B.format(256, 250)),
    ("hp=1", "rate=500", "band=8:30,sfreq=250", C.format(500, 250)),                                # a rate equal to sfreq is no stage
]


@pytest.mark.parametrize("iir,rs,pre,message", RATES)
def test_rate_rules_raise_the_same_string_from_the_chain_the_driver_and_the_data_set(shards, iir, rs, pre, message):
    import run as driver
    from data_provider.eeg_chain import EEGChain
    from data_provider.eeg_npy import EEGNpyDataset
    argv = ["--data", "EEG", "--data_root", str(shards.root), "--eeg_iir", iir, "--eeg_resample", rs, "--eeg_preprocess", pre]
    routes = (lambda: EEGChain(iir=iir, resample=rs, preprocess=pre).check("EEG"),
              lambda: driver.get_args(argv),
              lambda: EEGNpyDataset(str(shards.root), flag="val", chain=EEGChain(iir=iir, resample=rs, preprocess=pre)))
    for route in routes:
        if message is None:
            route()
        else:
            with pytest.raises(ValueError) as e:
                route()
            assert str(e.value) == message


def test_every_active_flag_needs_the_raw_chisco_shards(shards):
    from data_provider.eeg_chain import EEGChain
    said = {"preprocess": "--eeg_preprocess filters the raw CHISCO shards (--data EEG / EEG3), not --data UEA",
            "spatial": "--eeg_spatial acts on the electrodes of the raw CHISCO shards (--data EEG / EEG3), not --data UEA",
            "iir": "--eeg_iir filters the rows of the raw CHISCO shards (--data EEG / EEG3), not --data UEA",
            "resample": "--eeg_resample resamples the rows of the raw CHISCO shards (--data EEG / EEG3), not --data UEA"}
    texts = dict(preprocess="band=8:30", spatial="ref=car", iir="hp=1", resample="rate=256")
    for name, text in texts.items():
        with pytest.raises(ValueError) as e:
            EEGChain(**{name: text}).check("UEA")
        assert str(e.value) == said[name]
        EEGChain(**{name: text}).check("EEG3")
    EEGChain().check("UEA")
    with pytest.raises(ValueError) as e:                                # the driver's order: preprocess is named first
        EEGChain(**texts).check("SYNTH")
    assert str(e.value) == said["preprocess"].replace("UEA", "SYNTH")


class _Recorder:
    """the four stage ops and the standardisation, on CPU tensors: what was called, in which order, with what"""

    def __init__(self, monkeypatch, Cs):
        from ign_hip import ops
        self.calls = []
        for name in ("eeg_spatial", "eeg_iir", "eeg_resample", "eeg_filterbank", "standardise_nct_to_btc"):
            monkeypatch.setattr(ops, name, getattr(self, name))
        self.Cs = Cs

    def eeg_spatial(self, x, W, gid=None):
        self.calls.append(("eeg_spatial", x, W, gid))
        return x[:, :1].expand(-1, self.Cs, -1) + 1.0

    def eeg_iir(self, x, coef, pad, g0):
        self.calls.append(("eeg_iir", x, coef, dict(pad=pad, g0=g0)))
        return x + 2.0

    def eeg_resample(self, x, tab, up, down, half_len, edge):
        self.calls.append(("eeg_resample", x, tab, dict(up=up, down=down, half_len=half_len, edge=edge)))
        return x[:, :, :-(-x.shape[2] * up // down)] + 3.0

    def eeg_filterbank(self, x, taps, quad, decimate, edge, channels, timepoints):
        self.calls.append(("eeg_filterbank", x, taps, dict(quad=quad, decimate=decimate, edge=edge, channels=channels,
                                                            timepoints=timepoints)))
        return x.transpose(1, 2) + 4.0, torch.ones(x.shape[0], x.shape[2], dtype=torch.bool)

    def standardise_nct_to_btc(self, x):
        self.calls.append(("standardise", x, None, None))
        return x.transpose(1, 2) + 5.0


@pytest.mark.parametrize("pre", [False, True], ids=["standardise", "preprocess"])
def test_device_transform_calls_every_op_once_in_order_and_uploads_each_table_once(shards, monkeypatch, pre):
    from data_provider.data_factory import data_provider
    from exp.experiment_classification import Experiment
    rec = _Recorder(monkeypatch, 5)
    ds, loader = data_provider(_ns(shards, True, **_flags(shards, (True, True, True, pre))), "train")
    assert loader.eeg_chain is ds.chain and ds.chain.names == _names((True, True, True, pre))
    fitted = np.random.RandomState(3).randn(3, 5, 6).astype(np.float32)
    ds.spatial.W, ds.spatial.fitted = fitted, True                      # an alignment, assigned before the transform is built
    pf = Experiment._prefetch(Namespace(device=torch.device("cpu")), loader)
    assert pf.loader is loader
    torch.manual_seed(2)
    raw = list(loader)
    torch.manual_seed(2)
    got = list(pf)
    assert len(got) == len(raw) == 3
    tail = "eeg_filterbank" if pre else "standardise"
    assert [c[0] for c in rec.calls] == ["eeg_spatial", "eeg_iir", "eeg_resample", tail] * 3
    for b, (x, y, gid) in enumerate(raw):
        sp, iir, rs, last = rec.calls[4 * b:4 * b + 4]
        assert torch.equal(sp[1], x) and sp[1].dtype == torch.float32 and sp[3] is not None and torch.equal(sp[3], gid)
        assert gid.dtype == torch.int32 and torch.equal(sp[2], torch.from_numpy(fitted))       # W was read after the assignment
        assert torch.equal(iir[1], x[:, :1].expand(-1, 5, -1) + 1.0) and iir[3] == dict(pad=21, g0=ds.iir.g0)
        assert torch.equal(iir[2], torch.from_numpy(ds.iir.table)) and iir[2].dtype == torch.float64
        assert tuple(rs[1].shape) == (x.shape[0], 5, 400) and rs[3] == dict(up=64, down=125, half_len=ds.resample.hl, edge="reflect")
        assert torch.equal(rs[2], torch.from_numpy(ds.resample.tab))
        assert tuple(last[1].shape) == (x.shape[0], 5, 205)
        X, yb, mask = got[b]
        assert tuple(X.shape) == (x.shape[0], 205, 5) and torch.equal(yb, y) and tuple(mask.shape) == (x.shape[0], 205)
        assert mask.dtype == torch.bool and bool(mask.all())
        if pre:
            p = ds.pre
            assert torch.equal(last[2], torch.as_tensor(p.taps2d, dtype=torch.float32))
            assert last[3] == dict(quad=None, decimate=p.q, edge=p.edge, channels=p.Cout, timepoints=p.Tout)
    for k in range(4 if pre else 3):                                    # one table object per stage over the three batches
        assert len({id(rec.calls[4 * b + k][2]) for b in range(3)}) == 1


def test_gid_goes_to_the_spatial_stage_only_and_one_group_passes_none(shards, monkeypatch):
    from data_provider.eeg_chain import EEGChain
    rec = _Recorder(monkeypatch, 6)
    x, y, gid = torch.randn(4, 6, 400), torch.zeros(4, 1, dtype=torch.int64), torch.tensor([0, 2, 1, 0], dtype=torch.int32)
    one = EEGChain(spatial="ref=car", iir="hp=1").resolve(6, 400, str(shards.root), 24)
    one.device_transform("cpu")((x, y, gid))
    assert [c[0] for c in rec.calls] == ["eeg_spatial", "eeg_iir", "standardise"] and rec.calls[0][3] is None   # W holds one group
    del rec.calls[:]
    many = EEGChain(spatial="align=euclid", iir="hp=1", resample="rate=256", preprocess="band=8:30,sfreq=256")
    many = many.resolve(6, 400, str(shards.root), 24)
    many.stage("spatial").W = np.random.RandomState(1).randn(3, 6, 6).astype(np.float32)
    many.device_transform("cpu")((x, y, gid))
    assert [c[0] for c in rec.calls] == ["eeg_spatial", "eeg_iir", "eeg_resample", "eeg_filterbank"] and rec.calls[0][3] is gid
    for call in rec.calls[1:]:                                          # no later stage is handed the group ids
        assert not any(v is gid for v in (call[1], call[2], *call[3].values()))


def test_no_active_stage_is_the_standardisation_itself(shards):
    from data_provider import device_prefetch
    from data_provider.data_factory import data_provider
    from data_provider.eeg_chain import EEGChain
    from exp.experiment_classification import Experiment
    assert EEGChain().resolve(6, 400, str(shards.root), 24).device_transform("cpu") is device_prefetch.standardise_raw_batch
    for kw in ({}, _flags(shards, (False,) * 4), dict(eeg_resample="rate=500")):
        ds, loader = data_provider(_ns(shards, True, **kw), "test")
        assert loader.eeg_chain is ds.chain and ds.chain.stages == [] and ds.chain.shape == (6, 400)
        assert Experiment._prefetch(Namespace(device=torch.device("cpu")), loader).transform is device_prefetch.standardise_raw_batch


@pytest.mark.parametrize("on", COMBOS, ids=lambda on: "+".join(_names(on)) or "none")
def test_save_writes_exactly_the_records_of_the_active_stages(shards, tmp_path, on):
    from data_provider.eeg_chain import EEGChain
    f = _flags(shards, on)
    chain = EEGChain(**{k[len("eeg_"):]: v for k, v in f.items()}).resolve(6, 400, str(shards.root), 24)
    want = sorted(RECORDS[n] for n in _names(on) if n in RECORDS)
    assert sorted(os.path.basename(p) for p in chain.save(str(tmp_path))) == want == sorted(os.listdir(tmp_path))


def test_alignment_post_is_the_iir_stage_alone(shards):
    from data_provider.eeg_chain import EEGChain
    from utils.eeg_iir import iir_numpy
    root = str(shards.root)
    assert EEGChain(spatial="align=euclid", resample="rate=256").resolve(6, 400, root, 24).alignment_post("cpu") is None
    chain = EEGChain(spatial="align=euclid", iir="hp=1,notch=50", resample="rate=256").resolve(6, 400, root, 24)
    y = shards.X[:2].astype(np.float64)
    iir = chain.stage("iir")
    want = iir_numpy(y, iir.table, iir.pad, iir.g0)                     # float64, unrounded, the rows keep their length
    post = chain.alignment_post("cpu")
    assert post(y).tobytes() == want.tobytes() == post(torch.from_numpy(y)).tobytes() and want.shape == y.shape
