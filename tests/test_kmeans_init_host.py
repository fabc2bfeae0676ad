"""Shapelet initialisation by k-means (--shapelet_init kmeans), host side: the driver's flags, the seed draw, the refusals of
kmeans_init_ and of the ops on CPU tensors, and the argument errors of the three C entry points -- none of which needs a device."""
import ctypes
from argparse import Namespace

import pytest
import torch

from conftest import make_cfg

E_ARG, E_TOOBIG = -1001, -1003
P = ctypes.c_void_p(256)        # a non-null pointer that is never dereferenced: every call below fails validation first


def _lib():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import _lib
    return _lib.lib()


def test_flag_defaults_and_parser():
    import speech_imagery_eeg_amd  # noqa: F401
    import run
    a = run.get_args([])
    assert (a.shapelet_init, a.shapelet_init_iters, a.shapelet_init_batches) == ("normal", 10, 8)
    a = run.get_args(["--shapelet_init", "kmeans", "--shapelet_init_iters", "3", "--shapelet_init_batches", "2"])
    assert (a.shapelet_init, a.shapelet_init_iters, a.shapelet_init_batches) == ("kmeans", 3, 2)
    with pytest.raises(SystemExit):
        run.get_args(["--shapelet_init", "pca"])


def test_experiment_hook_does_nothing_by_default_and_on_models_without_shapelets(capsys):
    import speech_imagery_eeg_amd  # noqa: F401
    from exp.experiment_classification import Experiment
    from exp.experiment_regression import Experiment as RegressionExperiment
    assert RegressionExperiment._init_shapelets is Experiment._init_shapelets          # one hook, both harnesses
    e = Experiment.__new__(Experiment)
    e.rank = 0
    e.args = Namespace(model="SBM")                     # a namespace built without the new flags: the default
    e._init_shapelets()                                 # no model, no loader: must not touch either
    e.args = Namespace(model="DNN", shapelet_init="kmeans")
    e._init_shapelets()
    assert "no shapelets" in capsys.readouterr().out
    e.args = Namespace(model="SBM", shapelet_init="kmeans", test_only=True)
    e._init_shapelets()                                 # --test_only: nothing runs
    e.args = Namespace(model="SBM", shapelet_init="pca")
    with pytest.raises(ValueError):
        e._init_shapelets()


def test_seed_windows_are_distinct_reproducible_and_private():
    import speech_imagery_eeg_amd  # noqa: F401
    from utils.shapelet_init import draw_seed_windows
    torch.manual_seed(11)
    state = torch.get_rng_state()
    a = draw_seed_windows(7, 5, 40, torch.Generator().manual_seed(3))       # 5 of 7: collisions are certain to be drawn
    assert torch.equal(torch.get_rng_state(), state)                        # the global stream is not consumed
    assert a.shape == (5, 40) and a.dtype == torch.int64 and int(a.min()) >= 0 and int(a.max()) < 7
    assert all(len(set(a[:, c].tolist())) == 5 for c in range(40))
    assert torch.equal(a, draw_seed_windows(7, 5, 40, torch.Generator().manual_seed(3)))
    assert not torch.equal(a, draw_seed_windows(7, 5, 40, torch.Generator().manual_seed(4)))
    full = draw_seed_windows(5, 5, 3, torch.Generator().manual_seed(0))
    assert all(sorted(full[:, c].tolist()) == [0, 1, 2, 3, 4] for c in range(3))
    with pytest.raises(ValueError):
        draw_seed_windows(4, 5, 1, torch.Generator().manual_seed(0))


def test_kmeans_init_type_and_value_errors():
    import speech_imagery_eeg_amd  # noqa: F401
    from models.FullyConvNet import FullyConvNetwork
    from models.Shapelet import ShapeBottleneckModel
    from utils.shapelet_init import kmeans_init_
    x = torch.zeros(4, 100, 6)
    with pytest.raises(TypeError):
        kmeans_init_(torch.nn.Linear(3, 3), x)
    with pytest.raises(TypeError):
        kmeans_init_(FullyConvNetwork(make_cfg()), x)
    m = ShapeBottleneckModel(make_cfg(), [2], [0.1])
    with pytest.raises(ValueError):
        kmeans_init_(m, x, iters=0)
    with pytest.raises(ValueError):
        kmeans_init_(m, x[0])                           # not (n, T, C)


def test_ops_refuse_cpu_tensors():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    from ign_hip._lib import IgnError
    xn, w = torch.zeros(2, 3, 20), torch.zeros(4, 3, 5)
    with pytest.raises(IgnError):
        ops.shapelet_kmeans_step(xn, w)
    with pytest.raises(IgnError):
        ops.shapelet_kmeans_update(w, torch.zeros(4, 3, 5), torch.zeros(4, 3, dtype=torch.int32))


def test_workspace_query_answers_zero_outside_the_domain():
    L = _lib()
    assert L.ign_shapelet_kmeans_workspace_bytes(6, 3, 80, 4, 9, 1) > 0
    for bad in ((0, 3, 80, 4, 9, 1), (6, 0, 80, 4, 9, 1), (6, 3, 0, 4, 9, 1), (6, 3, 80, 0, 9, 1), (6, 3, 80, 4, 0, 1),
                (6, 3, 80, 4, 9, 0), (6, 3, 80, 4, 81, 1), (1, 1, 50000, 2, 10, 1)):
        assert L.ign_shapelet_kmeans_workspace_bytes(*bad) == 0, bad
    # assignments + per-row counts and minima + at least one slice of partial sums
    B, C, T, K, Lw = 6, 3, 80, 4, 9
    assert L.ign_shapelet_kmeans_workspace_bytes(B, C, T, K, Lw, 1) >= 4 * (B * C * (T - Lw + 1) + B * C * K + B * C + K * C * Lw)


def test_step_argument_errors():
    L = _lib()
    ok = (0, 6, 3, 80, 4, 9, 1)
    assert L.ign_shapelet_kmeans_step(P, P, None, P, P, P, P, 0, 6, 3, 80, 4, 81, 1, None) == E_ARG          # L > T
    assert L.ign_last_error().startswith(b"ign_shapelet_kmeans_step: bad dimensions")
    for dims in ((0, 3, 80, 4, 9, 1), (6, 0, 80, 4, 9, 1), (6, 3, 80, 0, 9, 1), (6, 3, 80, 4, 0, 1), (6, 3, 80, 4, 9, 0),
                 (6, 3, 80, 4, 9, -2)):
        assert L.ign_shapelet_kmeans_step(P, P, None, P, P, P, P, 0, *dims, None) == E_ARG, dims
    for null in (0, 1, 3, 4, 5, 6):                     # every pointer but `assign` (index 2) is required
        ptrs = [P, P, None, P, P, P, P]
        ptrs[null] = None
        assert L.ign_shapelet_kmeans_step(*ptrs, *ok, None) == E_ARG, null
        assert L.ign_last_error().startswith(b"ign_shapelet_kmeans_step: null pointer")
    assert L.ign_shapelet_kmeans_step(P, P, None, P, P, P, P, 2, *ok[1:], None) == E_ARG                     # accumulate flag
    assert L.ign_shapelet_kmeans_step(P, P, None, P, P, P, P, 0, 1, 1, 50000, 2, 10, 1, None) == E_TOOBIG    # the forward's row limit
    assert b"LDS" in L.ign_last_error()


def test_update_argument_errors():
    L = _lib()
    for dims in ((0, 3, 9), (4, 0, 9), (4, 3, 0)):
        assert L.ign_shapelet_kmeans_update(P, P, P, *dims, None) == E_ARG, dims
    for null in range(3):
        ptrs = [P, P, P]
        ptrs[null] = None
        assert L.ign_shapelet_kmeans_update(*ptrs, 4, 3, 9, None) == E_ARG
        assert L.ign_last_error().startswith(b"ign_shapelet_kmeans_update: null pointer")
