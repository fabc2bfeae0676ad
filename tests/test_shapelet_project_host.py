"""Shapelet projection (--shapelet_project), host side: the driver's flag and hook, the declaration / binding / export of the two
entry points of csrc/ign_shapelet_project.hip and their argument errors, the refusals of the ops and of project_, the ordered
loader, and the sidecar's round trip -- none of which needs a device.  The GPU side is tests/test_gpu_shapelet_project.py."""
import ctypes
import json
import os
import re
from argparse import Namespace

import pytest
import torch

from conftest import make_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1001
SYMBOLS = ("ign_shapelet_project_step", "ign_shapelet_project_step_bank")
P = ctypes.c_void_p(256)        # a non-null pointer that is never dereferenced: every call below fails validation first


def _mods():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops, _lib
    return ops, _lib


def _lib_or_skip():
    _, _lib = _mods()
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    return _lib.lib()


# ---------------------------------------------------------------- driver
def test_flag_default_and_parser():
    import speech_imagery_eeg_amd  # noqa: F401
    import run
    assert run.get_args([]).shapelet_project == "none"
    assert run.get_args(["--shapelet_project", "end"]).shapelet_project == "end"
    assert run.get_args(["--shapelet_project", "3"]).shapelet_project == 3
    for bad in ("0", "-1", "foo", "1.5", ""):
        with pytest.raises(SystemExit):
            run.get_args(["--shapelet_project", bad])
    assert "Adam" in run.build_parser().format_help()               # the help says that the moments are left alone


def test_hook_does_nothing_by_default_without_shapelets_and_under_test_only(capsys):
    import speech_imagery_eeg_amd  # noqa: F401
    from exp.experiment_classification import Experiment
    from exp.experiment_regression import Experiment as RegressionExperiment
    assert RegressionExperiment._project_shapelets is Experiment._project_shapelets         # one hook, both harnesses
    assert RegressionExperiment._project_final is Experiment._project_final
    e = Experiment.__new__(Experiment)
    e.rank = 0
    e.args = Namespace(model="SBM")                     # a namespace built without the flag: the default
    assert e._project_schedule() == (0, False)
    assert e._project_shapelets() is None               # no model, no loader: must not touch either
    assert e._project_summary() == {} and e._shapelet_sources_for_test() is None
    e.args = Namespace(model="SBM", shapelet_project="none")
    assert e._project_schedule() == (0, False) and e._project_shapelets() is None
    assert capsys.readouterr().out == ""
    for model in ("DNN", "EEGCNN"):
        e = Experiment.__new__(Experiment)
        e.rank = 0
        e.args = Namespace(model=model, shapelet_project="end")
        assert e._project_shapelets() is None and e._project_shapelets() is None
        assert e._project_final("checkpoint.pth") is None                                   # no validation pass, nothing saved
        assert capsys.readouterr().out.count("no shapelets") == 1                           # one notice
    e.args = Namespace(model="SBM", shapelet_project=2, test_only=True)
    assert e._project_schedule() == (2, True)
    assert e._project_shapelets() is None               # --test_only: nothing runs
    e.args = Namespace(model="SBM", shapelet_project="end")
    assert e._project_schedule() == (0, True)
    for bad in (0, -3, "often"):
        e.args = Namespace(model="SBM", shapelet_project=bad)
        with pytest.raises(ValueError):
            e._project_schedule()


def test_test_only_reads_the_sidecar(tmp_path):
    import speech_imagery_eeg_amd  # noqa: F401
    from exp.experiment_classification import Experiment
    from utils.shapelet_project import save_sources
    rep = _fake_report()
    save_sources(tmp_path / "shapelet_sources.json", rep)
    e = Experiment.__new__(Experiment)
    e.rank, e.checkpoint_dir = 0, str(tmp_path)
    e.args = Namespace(model="SBM", shapelet_project="end", test_only=True)
    src = e._shapelet_sources_for_test()
    assert torch.equal(src["source"], rep["source"]) and torch.equal(src["start"], rep["start"])
    row = e._project_summary()
    finite = rep["d_before"][torch.isfinite(rep["d_before"])]
    assert finite.numel() == 5 and row["shapelet_project"] == "end"
    assert abs(row["project_d_mean"] - float(finite.double().mean())) < 1e-12
    e.args = Namespace(model="SBM", test_only=True)                 # flag off: the file is not looked at
    assert e._shapelet_sources_for_test() is None and e._project_summary() == {}
    e.args = Namespace(model="SBM", shapelet_project="end")
    e.checkpoint_dir = str(tmp_path / "nowhere")
    assert e._shapelet_sources_for_test() is None and e._project_summary()["project_d_mean"] is None


# ---------------------------------------------------------------- ABI
def test_symbols_are_declared_bound_and_exported():
    ops, _lib = _mods()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    ctype_of = {"int": ctypes.c_int, "void*": ctypes.c_void_p}
    for name in SYMBOLS:
        m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        want = [ctypes.c_void_p if "*" in p else ctype_of[p.rsplit(" ", 1)[0]] for p in params]       # every pointer travels as void*
        assert res is ctypes.c_int and args == want, (name, params)
    src = open(os.path.join(ROOT, "speech-imagery-eeg_amd", "csrc", "ign_shapelet_project.hip")).read()
    for name in SYMBOLS:
        assert re.search(rf'extern "C" int {name}\(', src), name
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built")
    h = ctypes.CDLL(_lib.lib_path())
    for name in SYMBOLS:
        assert hasattr(h, name), name


def _step_args(**kw):
    a = dict(xn=P, dmin=P, tstar=P, ld=12, col0=0, sample0=0, best_d=P, best_src=P, cand=P, accumulate=0, B=6, C=3, T=80, K=4, L=9,
             stride=1, stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw,msg", [
    (dict(B=0), b"bad dimensions"), (dict(C=0), b"bad dimensions"), (dict(K=0), b"bad dimensions"), (dict(B=-2), b"bad dimensions"),
    (dict(T=0), b"bad dimensions"), (dict(L=0), b"bad dimensions"),
    (dict(L=81), b"bad dimensions"),                                # L > T
    (dict(stride=0), b"bad dimensions"), (dict(stride=-1), b"bad dimensions"),
    (dict(ld=11), b"row pitch"),                                    # ld < col0 + K*C
    (dict(col0=1), b"row pitch"), (dict(col0=-1), b"row pitch"),
    (dict(xn=None), b"null pointer"), (dict(dmin=None), b"null pointer"), (dict(tstar=None), b"null pointer"),
    (dict(best_d=None), b"null pointer"), (dict(best_src=None), b"null pointer"), (dict(cand=None), b"null pointer"),
    (dict(accumulate=2), b"accumulate"), (dict(sample0=-1), b"sample0"), (dict(sample0=2**31 - 3), b"sample0"),
])
def test_step_argument_errors(kw, msg):
    L = _lib_or_skip()
    assert L.ign_shapelet_project_step(*_step_args(**kw)) == E_ARG, kw
    err = L.ign_last_error()
    assert err.startswith(b"ign_shapelet_project_step: ") and msg in err, err


def _bank_args(G=2, **kw):
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)
    a = dict(xn=P, dmin=P, tstar=P, ld=21, G=G, col0=ints(0, 12), sample0=0, best_d=ptrs(256, 512), best_src=ptrs(256, 512),
             cand=ptrs(256, 512), accumulate=1, B=6, C=3, T=80, K=ints(4, 3), L=ints(9, 20), stride=ints(1, 2), stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return list(a.values())


def test_bank_validates_every_group_before_the_first_launch():
    L = _lib_or_skip()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)
    for kw, msg in ((dict(G=0), b"outside 1..8"), (dict(G=9), b"outside 1..8"), (dict(col0=None), b"null table"),
                    (dict(K=None), b"null table"), (dict(L=None), b"null table"), (dict(stride=None), b"null table"),
                    (dict(best_d=None), b"null table"), (dict(best_src=None), b"null table"), (dict(cand=None), b"null table"),
                    (dict(L=ints(9, 81)), b"bad dimensions"),        # the SECOND group is wrong: nothing may have been launched
                    (dict(stride=ints(1, 0)), b"bad dimensions"), (dict(K=ints(4, 0)), b"bad dimensions"),
                    (dict(ld=20), b"row pitch"), (dict(col0=ints(0, 13)), b"row pitch"),
                    (dict(cand=ptrs(256, None)), b"null pointer"), (dict(best_src=ptrs(256, None)), b"null pointer"),
                    (dict(xn=None), b"null pointer"), (dict(accumulate=-1), b"accumulate")):
        assert L.ign_shapelet_project_step_bank(*_bank_args(**kw)) == E_ARG, kw
        err = L.ign_last_error()
        assert err.startswith(b"ign_shapelet_project_step_bank: ") and msg in err, (kw, err)


# ---------------------------------------------------------------- ops and project_
def test_ops_refuse_cpu_tensors_and_bad_shapes():
    ops, _lib = _mods()
    xn, d, t = torch.zeros(2, 3, 20), torch.zeros(2, 12), torch.zeros(2, 12, dtype=torch.int32)
    with pytest.raises(_lib.IgnError):
        ops.shapelet_project_step(xn, d, t, 0, (4, 3, 5), 1, 0)
    with pytest.raises(_lib.IgnError):
        ops.shapelet_project_bank(xn, d, t, [(4, 3, 5)], [1], 0)
    with pytest.raises(_lib.IgnError):
        ops.shapelet_project_bank(xn, d, t, [(4, 3, 5)] * 9, [1] * 9, 0)        # above the bank limit: group by group, same refusal


def test_project_type_and_value_errors():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip._lib import IgnError
    from models.FullyConvNet import FullyConvNetwork
    from models.Shapelet import ShapeBottleneckModel
    from utils.shapelet_project import project_
    x = torch.zeros(4, 100, 6)
    with pytest.raises(TypeError):
        project_(torch.nn.Linear(3, 3), x)
    with pytest.raises(TypeError):
        project_(FullyConvNetwork(make_cfg()), x)
    m = ShapeBottleneckModel(make_cfg(), [2], [0.1])
    before = m.shapelets[0].weights.detach().clone()
    with pytest.raises(ValueError):
        project_(m, x[0])                               # not (n, T, C)
    with pytest.raises(ValueError):
        project_(m, [])                                 # no batches
    with pytest.raises(ValueError):
        project_(m, x[:0])
    if not torch.cuda.is_available():
        with pytest.raises(IgnError):                   # no CPU path
            project_(m, x)
    assert torch.equal(m.shapelets[0].weights, before)


# ---------------------------------------------------------------- ordered loader
class _Rows(torch.utils.data.Dataset):
    def __init__(self, n):
        self.x = torch.arange(n, dtype=torch.float32).reshape(n, 1, 1).expand(n, 5, 2).contiguous()
        self.y = torch.arange(n) % 3

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i], self.y[i]


def _collate(items):
    x = torch.stack([i[0] for i in items])
    return x, torch.stack([i[1] for i in items]).unsqueeze(1), torch.ones(x.shape[0], x.shape[1], dtype=torch.bool)


def _order(loader):
    return [int(v) for batch in loader for v in batch[0][:, 0, 0]]


def test_ordered_loader_yields_dataset_order_and_leaves_the_rng_alone():
    import speech_imagery_eeg_amd  # noqa: F401
    from data_provider.data_factory import RankShardSampler, ordered_loader
    from data_provider.device_prefetch import DevicePrefetcher, TensorBatchLoader
    ds = _Rows(23)
    shuffled = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=True, collate_fn=_collate)
    shuffled.eeg_chain = object()
    sharded = TensorBatchLoader(ds, 4, shuffle=True, sampler=RankShardSampler(23, 1, 2, True, seed=5), pin_memory=False)
    plain = TensorBatchLoader(ds, 4, shuffle=True, pin_memory=False)
    torch.manual_seed(3)
    assert all(_order(l) != list(range(23)) for l in (shuffled, sharded, plain))
    for src in (shuffled, sharded, plain, DevicePrefetcher(shuffled, "cpu", transform=lambda b: b)):
        state = torch.get_rng_state()
        out = ordered_loader(src)
        assert type(out) is type(src) and out is not src
        assert _order(out) == list(range(23)) and _order(out) == list(range(23))            # twice in a row
        assert torch.equal(torch.get_rng_state(), state)
        assert len(out) == 6 and [b[0].shape[0] for b in out] == [4, 4, 4, 4, 4, 3]
        inner = out.loader if isinstance(out, DevicePrefetcher) else out
        assert inner.batch_size == 4 and inner.dataset is ds
    out = ordered_loader(shuffled)
    assert out.collate_fn is _collate and out.eeg_chain is shuffled.eeg_chain
    assert next(iter(out))[2].dtype == torch.bool
    assert ordered_loader(plain).eeg_chain is None
    pre = ordered_loader(DevicePrefetcher(shuffled, "cpu", transform=_collate))
    assert pre.transform is _collate and pre.loader.collate_fn is _collate
    with pytest.raises(TypeError):
        ordered_loader([1, 2, 3])


# ---------------------------------------------------------------- sidecar
def _fake_report():
    src0 = torch.tensor([[[5, 7], [0, 0]], [[11, 3], [-1, -1]]], dtype=torch.int32)           # (K=2, C=2, 2); one shapelet kept
    d0 = torch.tensor([[0.25, 0.1], [1.0 / 3.0, float("inf")]])
    src1 = torch.tensor([[[2, 4], [9, 1]]], dtype=torch.int32)                                # (K=1, C=2, 2), stride 3
    d1 = torch.tensor([[0.5, 2.0]])
    groups = [dict(length=9, stride=1, source=src0, start=src0[..., 1].clone(), d_before=d0, kept=1),
              dict(length=20, stride=3, source=src1, start=src1[..., 1] * 3, d_before=d1, kept=0)]
    return dict(groups=groups, samples=12, batches=2, source=torch.cat([g["source"].reshape(-1, 2) for g in groups]),
                start=torch.cat([g["start"].reshape(-1) for g in groups]), d_before=torch.cat([g["d_before"].reshape(-1) for g in groups]))


def test_sidecar_round_trip(tmp_path):
    import speech_imagery_eeg_amd  # noqa: F401
    from utils.shapelet_project import load_sources, save_sources, sources_table
    rep = _fake_report()
    rows = sources_table(rep)
    assert [r["column"] for r in rows] == list(range(6))
    assert rows[1] == dict(column=1, group=0, k=0, c=1, index=0, window=0, start=0, length=9, d_before=float(rep["d_before"][1]))
    assert rows[3] == dict(column=3, group=0, k=1, c=1, index=-1, window=-1, start=-1, length=9, d_before=None)
    assert rows[5] == dict(column=5, group=1, k=0, c=1, index=9, window=1, start=3, length=20, d_before=2.0)
    path = save_sources(tmp_path / "shapelet_sources.json", rep)
    raw = json.load(open(path))                         # strict JSON: no Infinity / NaN literal
    assert raw["version"] == 1 and raw["samples"] == 12 and "Infinity" not in open(path).read()
    back = load_sources(path)
    assert torch.equal(back["source"], rep["source"]) and back["source"].dtype == torch.int32
    assert torch.equal(back["start"], rep["start"])
    assert torch.equal(back["d_before"], rep["d_before"])           # float32 -> JSON -> float32 is exact; the kept one is +inf
    assert back["length"].tolist() == [9, 9, 9, 9, 20, 20] and back["columns"] == rows
