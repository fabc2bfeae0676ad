"""Host-side checks of the wide class-head support (no GPU): the stated bound and the 39-class reference fixtures."""
import os
import re

import numpy as np

from conftest import ROOT, golden


def test_header_states_the_class_bound_and_python_agrees():
    src = open(os.path.join(ROOT, "include", "ign_abi.h")).read()
    m = re.search(r"#define\s+IGN_HEAD_NMAX\s+(\d+)", src)
    assert m and int(m.group(1)) >= 256
    ops_src = open(os.path.join(ROOT, "speech-imagery-eeg_amd", "ign_hip", "ops.py")).read()
    m2 = re.search(r"^HEAD_NMAX\s*=\s*(\d+)", ops_src, re.M)
    assert m2 and int(m2.group(1)) == int(m.group(1))


def test_many_class_fixtures_load_with_39_classes():
    g = golden("ign_fcn_n39")
    assert g["out"].shape == (8, 39) and g["sd.sbm.output_layer.weight"].shape[0] == 39
    assert g["sd.deep_model.fc.weight"].shape[0] == 39 and np.isfinite(g["train_loss"]).all()
    t = golden("train_step_ign_n39")
    assert t["sd0.deep_model.fc.weight"].shape[0] == 39 and t["losses"].shape == (3,)
    assert int(t["ys"].max()) < 39
    for name in ("ign_fcn_n39", "train_step_ign_n39"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1 << 20
