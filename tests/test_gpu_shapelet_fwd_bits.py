"""The shapelet forward, held to the bits of the library before its fixed-cost work (one-pass twin kernels with a ring window --
DESIGN 4.1d): that change moves instructions, not arithmetic, so every output must equal the recorded one bit for bit.

tests/golden/shapelet_fwd_parent_bits.npz was written by tests/gen_shapelet_fwd_parent_bits.py with that earlier library on an
MI355X, over tests/shapelet_fwd_bits_cases.py (B = 3, C = 2; the four benchmark variants, the window-count and tile edges, both
gates, the four distances, a periodic row for the first-index rule, and every TT with tiles 5 + 2 + 1).  Per case:
  1. p, dmin, tstar, zmu, d (and xstat) of ign_shapelet_fwd and of ign_shapelet_fwd_bank equal the fixture bitwise;
  2. independently of the fixture, they agree with the float64 oracle at 1e-4 element-wise;
  3. two calls give the same bits.
The variant a case runs is taken from the planner's rule (cases.variants mirrors fwd_staging / launch_fwd_group of csrc/ign_abi.hip
and the twin rule of shp_fwd_launch: the ABI has no forward-plan query), and every (TT, KT) pair instantiated in
csrc/ign_shapelet_fwd_p*.hip must be reached -- the plain kernel of each, and the twin of every TT that has one."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shapelet_fwd_bits_cases as S  # noqa: E402
from conftest import parity  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "shapelet_fwd_parent_bits.npz")
IDS = [c.name for c in S.CASES]
_RUNS, _FIX = {}, {}


def _fixture():
    if not _FIX:
        _FIX.update(np.load(FIXTURE, allow_pickle=False))
    return _FIX


def _run(case, entry, n=0):
    """Outputs of the n-th call of `entry` for a case; computed once per session and shared by the tests below."""
    key = (case.name, entry, n)
    if key not in _RUNS:
        assert torch.cuda.is_available(), "needs a GPU"
        import speech_imagery_eeg_amd  # noqa: F401
        _RUNS[key] = S.run(case, torch.device("cuda:0"), entry)
    return _RUNS[key]


# ---------------------------------------------------------------- coverage of the compiled variants (no device needed)
def _compiled_variants():
    tts, kts = set(), set()
    csrc = os.path.join(ROOT, "speech-imagery-eeg_amd", "csrc")
    for p in range(4):
        src = open(os.path.join(csrc, f"ign_shapelet_fwd_p{p}.hip")).read()
        table = src[src.index("ign_fwd_table_p"):]
        tts |= {int(t) for t in re.findall(r"IGN_FWD_ROW\((\d+)\)", table)}
        kts |= {int(k) for k in re.findall(r"shp_fwd_launch<TT, (\d+),", src)}
    return {(tt, kt) for tt in tts for kt in kts}


def test_every_compiled_variant_is_reached_by_a_case():
    """Plain kernels: every (TT, KT) of the tables, those beside a twin included; twins: every TT of FWD_TWIN_TTS."""
    compiled = _compiled_variants()
    assert compiled == {(tt, kt) for tt in range(1, 17) for kt in (1, 2, 5)}
    assert S.twin_tts() == [8, 11, 13, 15]
    reached = {v for c in S.CASES for v in S.variants(c)[0]}
    assert {(tt, kt) for tt, kt, twin in reached if not twin} == compiled
    assert {tt for tt, kt, twin in reached if twin} == set(S.twin_tts())
    by = {c.name: S.variants(c) for c in S.CASES}
    assert [by[f"bench_L{L}"][0] for L in (100, 200, 300, 500)] == [[(15, 5, True)], [(13, 5, True)], [(11, 5, True)], [(8, 5, True)]]
    assert [by[f"lts_L{L}"][0] for L in (100, 200, 300, 500)] == [[(15, 5, False)], [(13, 5, False)], [(11, 5, False)], [(8, 5, False)]]
    assert by["tw65"] == ([(2, 5, False)], 1) and by["tw64"] == ([(1, 5, False)], 1) and by["tw1"] == ([(1, 5, False)], 1)
    assert by["k7"][0] == [(5, 5, False), (5, 2, False)] and by["k1"][0] == [(3, 1, False)] and by["npass2"] == ([(16, 5, False)], 2)
    assert by["t1001"][0] == [(8, 5, True)] and by["lmod4"][0] == [(11, 5, True)] and by["nod_L300"][0] == [(11, 5, True)]
    assert by["tt16"][0] == [(16, 5, False), (16, 2, False), (16, 1, False)] and by["tt8"][0] == [(8, 5, True), (8, 2, False), (8, 1, False)]
    assert by["periodic_L500"][0] == [(8, 5, True)]


def test_fixture_holds_every_case():
    fix = _fixture()
    for c in S.CASES:
        want = {"p", "dmin", "tstar", "zmu"} | ({"d_ck"} | ({"d"} if c.full else set()) if c.want_d else set()) \
            | ({"xstat"} if c.mode & 0xf >= S.COS else set())
        assert {k.split("/")[1] for k in fix if k.split("/")[0] == c.name} == want, c.name
    assert os.path.getsize(FIXTURE) < 1 << 20


# ---------------------------------------------------------------- 1. the parent's bits
@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["single", "bank"])
@pytest.mark.parametrize("name", IDS)
def test_outputs_are_bitwise_the_recorded_ones(name, entry):
    case, fix = S.BY_NAME[name], _fixture()
    got = S.stored(case, _run(case, entry))
    assert sorted(got) == sorted(k for k in fix if k.split("/")[0] == name)
    for k, v in got.items():
        assert v.dtype == fix[k].dtype and v.shape == fix[k].shape, k
        diff = int((v.view(np.uint32) != fix[k].view(np.uint32)).sum())
        assert diff == 0, f"{k}: {diff} of {v.size} words differ"


# ---------------------------------------------------------------- 2. the float64 oracle
def _oracle(case):
    from oracle import ign_oracle as O
    xn, w, thr = S.inputs(case)
    d = O.window_distance(xn.double(), w.double(), 1, case.mode & 0xf, chunk=64)          # (B, Tw, K, C)
    dmin = d.min(dim=1).values
    if case.mode & S.LTS:
        e = torch.exp(dmin.unsqueeze(1) - d)
        Z, mu = e.sum(1), (e * d).sum(1) / e.sum(1)
        p = torch.sigmoid(thr.double().unsqueeze(0) - dmin)
    else:
        pt = torch.exp(-(S.EPS * d) ** 2)
        e = torch.exp(pt)
        Z, mu = e.sum(1), (e * pt).sum(1) / e.sum(1)
        p = pt.max(dim=1).values
    return dict(d=d.permute(0, 3, 2, 1), dmin=dmin.flatten(1), p=p.flatten(1), zmu=torch.stack([Z, mu], dim=-1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_outputs_match_the_float64_oracle(name):
    case = S.BY_NAME[name]
    got, ref = _run(case, "single"), _oracle(case)
    for k in ("p", "dmin", "zmu") + (("d",) if case.want_d else ()):
        parity(f"{name} {k}", got[k], ref[k], tol=1e-4, kind="elem", ref_is="float64 oracle")
    # the window picked: through the distances, as a window that ties the optimum to the last fp32 bit may be picked instead
    d = ref["d"].permute(0, 2, 1, 3)                                                      # (B, K, C, Tw)
    t = torch.from_numpy(got["tstar"]).long()
    assert int(t.min()) >= 0 and int(t.max()) < d.shape[-1]
    picked = d.gather(3, t.unsqueeze(-1)).squeeze(-1)
    assert float((picked - d.min(dim=3).values).abs().max()) <= 1e-5
    if case.x == "periodic":                          # every window recurs 50 samples later, bit for bit: the first one wins
        assert int(t.max()) < 50
        assert int(t[S.B - 1, 0].max()) == 0 and float(np.abs(got["dmin"].reshape(S.B, case.K, S.C)[S.B - 1, 0]).max()) == 0.0
    if "xstat" in got:
        xn = S.inputs(case)[0].double()
        win = xn.unfold(2, case.L, 1)                                                     # (B, C, Tw, L)
        if case.mode & 0xf == S.PEARSON:
            win = win - win.mean(dim=-1, keepdim=True)
        parity(f"{name} xstat", got["xstat"], win.pow(2).sum(-1).sqrt(), tol=1e-4, kind="elem", ref_is="float64 oracle")


# ---------------------------------------------------------------- 3. repeatability
@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_two_calls_give_the_same_bits(name):
    case = S.BY_NAME[name]
    a, b = _run(case, "single"), _run(case, "single", 1)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
