"""Every output bit of the cross-entropy loss tail (ops.ign_loss under its three label rules, both kernel layouts) against
tests/golden/loss_tail_bits.json: sha256 digests recorded on the MI355X from the six hand-written kernels that the two kernel
templates over a label rule replaced (the file names the git blob of that csrc/ign_loss.hip, the HIP and the torch version).  The
cases, their grid and the reason for every size are tests/diag_loss_tail.py's (ce_cases); re-record with
`python tests/diag_loss_tail.py --digest tests/golden/loss_tail_bits.json` on a checkout of the commit whose bits are to be pinned."""
import json
import os

import pytest
import torch

import diag_loss_tail as D

pytestmark = pytest.mark.gpu
CASES = {tag: (x, options) for tag, x, options in D.ce_cases()}
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_tail_bits.json")) as f:
    GOLDEN = json.load(f)


def test_fixture_covers_the_grid():
    assert (GOLDEN["beta"], GOLDEN["reg"]) == (D.CE_BETA, D.CE_REG)
    assert {t: sorted(c["outputs"]) for t, c in GOLDEN["cases"].items()} == {t: sorted(o) for t, (_, o) in CASES.items()}
    assert all(sorted(o) == sorted(D.CE_OUTPUTS) for c in GOLDEN["cases"].values() for o in c["outputs"].values())


@pytest.mark.parametrize("tag", sorted(CASES))
def test_bits_are_the_recorded_ones(tag):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    x, options = CASES[tag]
    want = GOLDEN["cases"][tag]
    inputs = {k: D.sha(v) for k, v in x.items()}
    assert inputs == want["inputs"], (f"{tag}: the inputs differ from the recorded ones ({[k for k in inputs if inputs[k] != want['inputs'].get(k)]}): "
                                      f"the fixture was recorded under a different generator (torch {GOLDEN['torch']}, here {torch.__version__}) "
                                      "and must be re-recorded from the parent commit")
    got = D.ce_digests(ops, torch.device("cuda:0"), x, options)["outputs"]
    bad = [f"{o}.{n}" for o in options for n in D.CE_OUTPUTS if got[o][n] != want["outputs"][o][n]]
    assert not bad, f"{tag}: bits differ from the recorded ones in {bad}"
