"""Host-side checks of the FCN expert's input gradient (no GPU): the CPU oracle reproduces the reference fixture
(tests/golden/make_golden_fcn_input_grad.py) through its own autograd, utils.saliency.input_saliency refuses bad `explain`
arguments before any device work, and the four ign_clconv_dgrad_input* entry points are declared and bound alike."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden, make_cfg, sd_from

NEW = ["ign_clconv_dgrad_input", "ign_clconv_dgrad_input_x6", "ign_clconv_dgrad_input_bf16", "ign_clconv_dgrad_input_h3"]


def _rel_to_max(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(got.detach().double().numpy() - ref).max() / max(np.abs(ref).max(), 1e-30))


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_oracle_reproduces_the_fixture(mode):
    """a restatement agrees with the reference to 1e-6 of the maximum (both float32 on the CPU)."""
    from oracle import ign_oracle as O
    g = golden("ign_fcn_input_grad")
    x = torch.from_numpy(g["x"])
    B, T, C = x.shape
    N = g[f"{mode}.out"].shape[1]
    m = O.OracleIGN(make_cfg(enc_in=C, seq_len=T, num_class=N, c_out=N, dec_in=C))
    m.load_state_dict(sd_from(g))
    m.train(mode == "train")
    xg = x.clone().requires_grad_(True)
    out, info = m(xg)
    gx, = torch.autograd.grad(out.sum(), xg, retain_graph=True)
    gd, = torch.autograd.grad(info.dnn_preds.sum(), xg)
    for name, got in (("out", out), ("eta", info.eta), ("dnn_preds", info.dnn_preds), ("grad_x", gx), ("grad_x_dnn", gd)):
        err = _rel_to_max(got, g[f"{mode}.{name}"])
        print(f"{mode}.{name}: {err:.3e}")
        assert err <= 1e-6, (mode, name, err)


def test_fixture_has_running_statistics_and_stays_small():
    g = golden("ign_fcn_input_grad")
    assert float(np.abs(g["sd.deep_model.block1.1.running_mean"]).max()) > 1e-3
    assert float(np.abs(g["sd.deep_model.block2.1.running_var"] - 1.0).max()) > 1e-3
    assert int(g["sd.deep_model.block1.1.num_batches_tracked"]) == 3
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ign_fcn_input_grad.npz")) < (1 << 20)
    assert not np.array_equal(g["eval.grad_x"], g["train.grad_x"])


def test_input_saliency_rejects_bad_explain_before_any_device_work():
    import speech_imagery_eeg_amd  # noqa
    from models.Shapelet import ShapeBottleneckModel
    from utils.saliency import input_saliency
    m = ShapeBottleneckModel(make_cfg(enc_in=3, seq_len=40, num_class=2, c_out=2, dec_in=3))
    x = torch.randn(2, 40, 3)                                          # a CPU tensor: any device work would raise IgnError
    with pytest.raises(ValueError, match="explain"):
        input_saliency(m, x, explain="mixture")
    with pytest.raises(TypeError, match="FCN"):
        input_saliency(m, x, explain="dnn")
    with pytest.raises(TypeError, match="FCN"):
        input_saliency(m, x, explain="gated")
    assert m.training and all(p.requires_grad for p in m.parameters())


def test_header_and_binding_list_the_four_entry_points():
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ign_abi.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, f"{name} not declared"
        params = [p.strip() for p in m.group(1).split(",")]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params), name
        assert params[-1] == "void* stream" and [p.split()[-1] for p in params[-6:-1]] == ["B", "Tin", "Ci", "Co", "k"]
    assert set(ops._CLCONV_DGRAD_INPUT.values()) == set(NEW)
    assert [p.strip().split()[-1] for p in re.search(r"ign_clconv_dgrad_input_h3\s*\(([^)]*)\)", hdr).group(1).split(",")][3:5] \
        == ["bound_dy", "bound_w"]


def test_argument_errors_are_reported_without_touching_a_device():
    import ctypes
    import speech_imagery_eeg_amd  # noqa
    from ign_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        pytest.skip("libign_hip.so not built (run __graft_entry__.build())")
    L = _lib.lib()
    ARG, UNSUP = -1001, -1002
    pp = ctypes.c_void_p(0x1000)                                       # never dereferenced: every call below is refused on the host
    assert L.ign_clconv_dgrad_input(None, pp, pp, 1, 16, 3, 4, 3, None) == ARG
    assert L.ign_clconv_dgrad_input_x6(pp, pp, None, 1, 16, 3, 4, 3, None) == ARG
    assert L.ign_clconv_dgrad_input_bf16(pp, pp, pp, 1, 2, 3, 4, 3, None) == ARG          # Tout <= 0
    assert L.ign_clconv_dgrad_input(pp, pp, pp, 1, 16, 0, 4, 3, None) == ARG              # Ci >= 1
    assert L.ign_clconv_dgrad_input_h3(pp, pp, pp, pp, None, 1, 16, 3, 4, 3, None) == ARG
    assert b"null operand bound" in L.ign_last_error()
    assert L.ign_clconv_dgrad_input(pp, pp, pp, 1, 16, 3, 6, 3, None) == UNSUP            # Co % 4
    assert b"Co % 4" in L.ign_last_error()
    assert L.ign_clconv_dgrad_input_x6(pp, pp, pp, 1, 40, 3, 4, 17, None) == UNSUP         # k <= 16 on the split kernels
    assert L.ign_clconv_dgrad_input_h3(pp, pp, pp, pp, pp, 1, 40, 3, 4, 17, None) == UNSUP
