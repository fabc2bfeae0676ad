"""IGN_TIE_EXACT (mode bit 0x20: the L1 backward passes take sign(0) = 0 at x == w, as aten::sgn), host side: the constant in the
header and in ops, which modes the entry points accept, Shapelet.mode() / tie_exact / set_tie_exact, and the bit travelling unchanged
through the three bank launchers.  Needs no device; the GPU side is tests/test_gpu_tie_exact.py."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import make_cfg
from test_shapelet_host import (B, C, T, LTS, RBF, L1, MSE, COS, _bank, _col0, _common, _forward, _named, _p as _ptrs, _saved, _wgrad,
                                _xgrad, host)  # noqa: F401  (host: the stand-in library fixture)
from test_input_grad_host import E_ARG, _grp_args, _lib_or_skip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE = 0x20


# ---------------------------------------------------------------- constants
def test_constants_agree():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    hdr = open(os.path.join(ROOT, "include", "ign_abi.h")).read()
    assert re.search(r"^#define\s+IGN_TIE_EXACT\s+0x20\b", hdr, flags=re.M)
    assert ops.TIE_EXACT == TIE
    assert TIE & (0xf | ops.GATE_LTS) == 0                                  # a bit of its own, outside the distance nibble and the gate
    assert _lib_or_skip().ign_abi_version() == 1


def test_header_describes_the_switch_in_both_convention_paragraphs():
    hdr = open(os.path.join(ROOT, "include", "ign_abi.h")).read()
    w_doc = hdr[hdr.index("sign(0) convention (IGN_DIST_L1 only).  The reference"):hdr.index("size_t ign_shapelet_bwd_workspace_bytes(")]
    x_doc = hdr[hdr.index("Backward of ign_shapelet_fwd w.r.t. the INPUT"):hdr.index("int ign_shapelet_bwd_input(")]
    for doc in (w_doc, x_doc):
        assert "IGN_TIE_EXACT" in doc and "contributes 0" in doc and "aten::sgn" in doc
    assert "sign(0) convention" in x_doc and "sign(x - w) = -1" in x_doc     # the existing sentences stay


# ---------------------------------------------------------------- mode validation (everything returns before a launch)
@pytest.mark.parametrize("kw,msg", [
    (dict(mode=TIE, gx=None), b"null pointer"),
    (dict(mode=TIE | 0x10, p=None), b"null pointer"),
    (dict(mode=0x40), b"unknown mode"),
    (dict(mode=0x64), b"unknown mode"),
    (dict(mode=0x22), b"IGN_DIST_L1 and IGN_DIST_MSE only"),
])
def test_input_pass_accepts_the_bit_and_nothing_above_it(kw, msg):
    L = _lib_or_skip()
    assert L.ign_shapelet_bwd_input(*_grp_args(**kw)) == E_ARG
    err = L.ign_last_error()
    assert msg in err and (msg == b"unknown mode" or b"unknown mode" not in err)


def test_weight_pass_and_forward_accept_the_bit():
    """a null pointer is reported (the mode passed), 0x60 is an unknown mode; the workspace of the fixture shape is non-zero"""
    L = _lib_or_skip()
    p = ctypes.c_void_p
    for mode, msg in ((TIE, b"null pointer"), (TIE | 0x10, b"null pointer"), (TIE | 0x40, b"unknown mode")):
        rc = L.ign_shapelet_bwd(p(16), p(32), p(48), p(64), p(80), 12, 0, p(96), p(112), p(128), None, None, None, p(160), 2, 4, 60, 3, 9, 1,
                                1.0, mode, None)
        assert rc == E_ARG and msg in L.ign_last_error(), mode
        rc = L.ign_shapelet_fwd(p(16), p(32), p(48), None, p(64), 12, 0, p(80), p(96), None, None, 2, 4, 60, 3, 9, 1, 1.0, mode, None)
        assert rc == E_ARG and msg in L.ign_last_error(), mode
    for mode in (TIE, TIE | 0x10):
        n = L.ign_shapelet_bwd_workspace_bytes(3, 4, 60, 3, 9, 1, mode)
        assert n != 0 and n == L.ign_shapelet_bwd_workspace_bytes(3, 4, 60, 3, 9, 1, mode & ~TIE)      # same plan, same partial buffer
    it = ctypes.c_int * 1
    assert L.ign_shapelet_bwd_bank_workspace_bytes(1, 3, 4, 60, it(3), it(9), it(1), TIE) != 0


# ---------------------------------------------------------------- Shapelet.mode()
def _models():
    import speech_imagery_eeg_amd  # noqa: F401
    from models import Shapelet as S
    return S


def test_mode_carries_the_bit_for_l1_only_and_not_by_default():
    S = _models()
    if os.environ.get("IGN_TIE_EXACT") != "1":
        assert S.Shapelet.tie_exact is False
        assert S.Shapelet(3, 9, 2).mode() == L1 | RBF and S.DistThresholdShapelet(3, 9, 2).mode() == L1 | LTS
    for cls, gate in ((S.Shapelet, RBF), (S.DistThresholdShapelet, LTS)):
        s = cls(3, 9, 2)
        s.tie_exact = True
        assert s.mode() == L1 | gate | TIE
        s.tie_exact = False
        assert s.mode() == L1 | gate
        m = cls(3, 9, 2, memory_efficient=True)
        m.tie_exact = True
        assert m.mode() == MSE | gate
    for dfunc in ("cosine", "pearson"):
        s = S.Shapelet(3, 9, 2, distance_func=dfunc)
        s.tie_exact = True
        assert s.mode() & TIE == 0 and s.mode() & 0xf >= COS


@pytest.mark.parametrize("env,want", [("1", True), ("0", False), (None, False)])
def test_class_default_is_read_from_the_environment_on_import(env, want):
    e = {k: v for k, v in os.environ.items() if k != "IGN_TIE_EXACT"}
    if env is not None:
        e["IGN_TIE_EXACT"] = env
    code = "import speech_imagery_eeg_amd; from models.Shapelet import Shapelet; print('TIE', Shapelet.tie_exact, hex(Shapelet(3, 9, 2).mode()))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"TIE {want} {hex(TIE if want else 0)}" in r.stdout


@pytest.mark.parametrize("cls_name", ["ShapeBottleneckModel", "DistThresholdSBM"])
def test_set_tie_exact_reaches_every_group(cls_name):
    S = _models()
    m = getattr(S, cls_name)(make_cfg(enc_in=3, seq_len=60, num_class=3), num_shapelet=[2] * 4)
    gate = LTS if cls_name == "DistThresholdSBM" else RBF
    assert m.set_tie_exact(True) is m
    assert [s.mode() for s in m.shapelets] == [L1 | gate | TIE] * 4
    m.set_tie_exact(False)
    assert [s.mode() for s in m.shapelets] == [L1 | gate] * 4
    assert "tie_exact" not in m.state_dict() and not any("tie_exact" in k for k in m.state_dict())


def test_interpgn_reaches_the_switch_through_its_sbm():
    import speech_imagery_eeg_amd  # noqa: F401
    from models.InterpGN import InterpGN
    m = InterpGN(make_cfg(enc_in=3, seq_len=60, num_class=3))
    m.sbm.set_tie_exact(True)
    assert all(s.mode() & TIE for s in m.sbm.shapelets)


# ---------------------------------------------------------------- the launchers pass the bit
def _calls(ops, rec, labels, G, mode):
    """one forward, weight-gradient and input-gradient launch of a G-group bank in `mode`: -> the recorded calls with every device
    address replaced by its position in the list of distinct addresses (the tensors differ from run to run, their roles do not)"""
    del rec.calls[:], labels[:]
    xn, ws, thrs, Ks, Ls, strides = _bank(G, mode)
    bank, P, D = _forward(ops, xn, ws, thrs, mode, strides, True)
    gP = torch.randn(B, sum(Ks) * C, generator=torch.Generator().manual_seed(1))
    _wgrad(ops, bank, xn, gP, P, D)
    _xgrad(ops, bank, xn, gP, P, D)
    return list(rec.calls), list(labels), (xn, ws, thrs, Ks, Ls, strides, bank, P, D, gP)


@pytest.mark.parametrize("base", [L1 | RBF, L1 | LTS, MSE | LTS])
@pytest.mark.parametrize("G", [1, 4, 9])
def test_launchers_pass_the_bit_unchanged(host, G, base):
    ops, _lib, rec, labels = host
    plain, plain_labels, _ = _calls(ops, rec, labels, G, base)
    tied, tied_labels, (xn, ws, thrs, Ks, Ls, strides, bank, P, D, gP) = _calls(ops, rec, labels, G, base | TIE)
    assert bank.mode == base | TIE
    assert tied_labels == plain_labels and [n for n, _ in tied] == [n for n, _ in plain]
    names = {n for n, _ in tied}
    assert names == ({"ign_shapelet_fwd_bank", "ign_shapelet_bwd_bank_workspace_bytes", "ign_shapelet_bwd_bank", "ign_shapelet_bwd_input_bank"}
                     if G <= 8 else {"ign_shapelet_fwd", "ign_shapelet_bwd_workspace_bytes", "ign_shapelet_bwd", "ign_shapelet_bwd_input"})
    for (name, a_t), (_, a_p) in zip(tied, plain):
        got_t, got_p = _named(_lib, (name, a_t), name), _named(_lib, (name, a_p), name)
        assert got_t["mode"] == base | TIE and got_p["mode"] == base, name
        # every other argument as without the bit: the same numbers and tables; addresses are null in the same places
        for k in got_p:
            if k == "mode":
                continue
            vt, vp = got_t[k], got_p[k]
            if isinstance(vp, list) and k not in ("K", "L", "stride", "col0"):
                assert [v is None for v in vt] == [v is None for v in vp], (name, k)
            elif isinstance(vp, (float,)) or k in ("K", "L", "stride", "col0", "G", "B", "C", "T", "ld", "accumulate", "stream"):
                assert vt == vp, (name, k)
            else:
                assert (vt is None) == (vp is None), (name, k)
    # and the addresses of the run with the bit are the bank's own
    sv = [_saved(bank, g) for g in range(G)]
    tstar, zmu, dsave, xstat, col0 = [list(f) for f in zip(*sv)]
    assert col0 == _col0(Ks)
    common = _common(xn, P, D, Ks, base | TIE)
    if G <= 8:
        fwd = _named(_lib, tied[0], "ign_shapelet_fwd_bank")
        assert fwd == dict(common, G=G, w_kcl=_ptrs(ws), thr_kc=_ptrs(thrs), col0=col0, tstar=_ptrs(tstar), zmu=_ptrs(zmu),
                           d_save=_ptrs(dsave), xstat_save=_ptrs(xstat), K=Ks, L=Ls, stride=strides)
        size = _named(_lib, tied[1], "ign_shapelet_bwd_bank_workspace_bytes")
        assert size == dict(G=G, B=B, C=C, T=T, K=Ks, L=Ls, stride=strides, mode=base | TIE)
        xg = _named(_lib, tied[3], "ign_shapelet_bwd_input_bank")
        gx = xg.pop("gxn_bct")
        assert gx is not None and xg == dict(common, g_out=gP.data_ptr(), G=G, w_kcl=_ptrs(ws), col0=col0, tstar=_ptrs(tstar), zmu=_ptrs(zmu),
                                             d_save=_ptrs(dsave), K=Ks, L=Ls, stride=strides)
    else:
        for g in range(G):
            fwd = _named(_lib, tied[g], "ign_shapelet_fwd")
            assert fwd == dict(common, w_kcl=ws[g].data_ptr(), thr_kc=_ptrs(thrs)[g], col0=col0[g], tstar=tstar[g].data_ptr(),
                               zmu=zmu[g].data_ptr(), d_save=dsave[g].data_ptr(), xstat_save=_ptrs(xstat)[g], K=Ks[g], L=Ls[g],
                               stride=strides[g])
            size = _named(_lib, tied[G + 2 * g], "ign_shapelet_bwd_workspace_bytes")
            assert size == dict(B=B, C=C, T=T, K=Ks[g], L=Ls[g], stride=strides[g], mode=base | TIE)
            assert _named(_lib, tied[G + 2 * g + 1], "ign_shapelet_bwd")["mode"] == base | TIE
            xg = _named(_lib, tied[3 * G + g], "ign_shapelet_bwd_input")
            assert xg["mode"] == base | TIE and xg["accumulate"] == (1 if g else 0) and xg["K"] == Ks[g] and xg["L"] == Ls[g]
