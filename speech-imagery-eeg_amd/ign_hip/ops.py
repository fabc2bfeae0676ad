"""Autograd ops over the C ABI (include/ign_abi.h).  torch supplies device memory, streams and autograd
plumbing; the arithmetic is in libign_hip.so.  Every op raises on CPU tensors: there is no fallback path."""
import ctypes
from collections import namedtuple

import torch

from . import _lib

import os

DIST_L1, DIST_MSE, DIST_COS, DIST_PEARSON = 0, 1, 2, 3
ATTN_MATH = os.environ.get("IGN_ATTN_MATH", "bf16x6")          # "f32": attention core on the fp32-MFMA kernels
LAYERNORM_MIN_ROWS = 0        # round 1 kept torch below 64k rows; with the row-count-aware grid and the parallel reduce the HIP kernels win everywhere
LINEAR_WGRAD = "bf16x6"       # weight gradient of ops.linear on the split kernels; "f32" (set by tests / diag scripts): the fp32-MFMA TN kernel
GATE_RBF, GATE_LTS = 0x00, 0x10
TIE_EXACT = 0x20              # IGN_TIE_EXACT: the L1 backward passes take sign(0) = 0 at x == w, as aten::sgn; travels inside `mode`
HEAD_NMAX = 256               # IGN_HEAD_NMAX (include/ign_abi.h): widest class head of ign_head_* / ign_loss_*
NO_WINDOW = 1e18             # Dmin of a feature without a valid window under `lengths` (IGN_NO_WINDOW, csrc/ign_shapelet_mask.hip); its Tstar is -1
HEAD_WIDE_BMAX = 640          # batch bound of ign_head_bwd above 16 classes (one 16-class chunk of the logit gradient in 40 KB of LDS)


def head_fits(B, N):
    """Whether ign_head_fwd / ign_head_bwd take a (B, N) head.  N <= 16 keeps its own rule (checked by the kernel)."""
    return N <= 16 or (N <= HEAD_NMAX and B <= HEAD_WIDE_BMAX)


def _check_classes(name, n):
    if n > HEAD_NMAX:
        raise _lib.IgnError(f"{name}: N={n} classes > {HEAD_NMAX}, the widest class head the HIP kernels take (IGN_HEAD_NMAX)")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


_stream = _lib.stream


def _need_gpu(name, *ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.IgnError(f"{name}: tensor on {t.device}; the IGN hot path runs on the MI355X only "
                                f"(no CPU fallback -- the CPU restatement lives in oracle/ for tests)")
        if t.dtype != torch.float32:
            raise _lib.IgnError(f"{name}: expected float32, got {t.dtype}")


def instance_norm(x_btc, want_raw=False, eps=1e-8, input_bound=False):
    """(B,T,C) -> normalised (B,C,T) [+ raw transpose].  Replaces IGN/model/Shapelet.py:186-187.
    `input_bound`: also attach max |x| to `x_btc` (see cached_bound) for a consumer of the raw batch.
    An autograd node (InstanceNormFn) when, and only when, `x_btc` requires a gradient and grad mode is on; the training step,
    whose inputs are data, runs the plain pass below."""
    if x_btc.requires_grad and torch.is_grad_enabled():
        _need_gpu("instance_norm", x_btc)
        xn, xt = InstanceNormFn.apply(x_btc, want_raw, eps, input_bound)
        return xn, xt
    return _instance_norm(x_btc, want_raw, eps, input_bound)


def _instance_norm(x_btc, want_raw, eps, input_bound):
    _need_gpu("instance_norm", x_btc)
    x = x_btc.contiguous()
    B, T, C = x.shape
    xn = torch.empty(B, C, T, device=x.device, dtype=torch.float32)
    xt = torch.empty_like(xn) if want_raw else None
    L = _lib.lib()
    if input_bound and cached_bound(x_btc) is None:
        # the raw batch is staged in LDS by this pass anyway: take max |x| here, for the FCN expert's first fp16 GEMM
        # (ign_hip/fcn.py looks the bound up on the tensor) instead of a separate pass over x
        slot = _new_slot(x.device)
        _lib.check(L.ign_instnorm_fwd_amax(_ptr(x), _ptr(xn), _ptr(xt), B, T, C, eps, _ptr(slot), _stream()), "ign_instnorm_fwd_amax")
        set_bound(x_btc, slot)
    else:
        _lib.check(L.ign_instnorm_fwd(_ptr(x), _ptr(xn), _ptr(xt), B, T, C, eps, _stream()), "ign_instnorm_fwd")
    return xn, xt


def _lengths(name, lengths, B):
    """The per-sample lengths of a zero-padded batch as the kernels take them: a contiguous int32 (B) tensor on the GPU."""
    if not torch.is_tensor(lengths) or not lengths.is_cuda or lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,):
        what = f"{lengths.dtype} {tuple(lengths.shape)} on {lengths.device}" if torch.is_tensor(lengths) else type(lengths).__name__
        raise _lib.IgnError(f"{name}: lengths must be an int32 tensor of shape ({B},) on the GPU, got {what}")
    return lengths.contiguous()


def _no_input_grad_with_lengths(name, needs_grad):
    if needs_grad:
        raise _lib.IgnError(f"{name}: the input requires a gradient, but there is no length-aware ign_instnorm_bwd: input gradients "
                            f"(saliency) run without `lengths`, on the padded batch")


def instance_norm_len(x_btc, lengths, eps=1e-8):
    """instance_norm for a batch zero-padded at the end: sample b has lengths[b] (int32, on the GPU) samples of data.  Mean and
    unbiased std over x[b, :n_b] only; -> normalised (B,C,T) with exact zeros from n_b on (a row with n_b < 2 is all zeros).
    No raw transpose, no input bound, no gradient (ign_instnorm_fwd_len)."""
    name = "instance_norm_len"
    _need_gpu(name, x_btc)
    _no_input_grad_with_lengths(name, x_btc.requires_grad and torch.is_grad_enabled())
    x = x_btc.detach().contiguous()
    B, T, C = x.shape
    lengths = _lengths(name, lengths, B)
    xn = torch.empty(B, C, T, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().ign_instnorm_fwd_len(_ptr(x), _ptr(lengths), _ptr(xn), B, T, C, eps, _stream()), "ign_instnorm_fwd_len")
    return xn


class InstanceNormFn(torch.autograd.Function):
    """instance_norm for an input that requires a gradient: the same forward launch; the backward recomputes mean and std from
    x (ign_instnorm_bwd -- the forward saves no statistics) and returns the gradient in the loader's (B,T,C) layout.  A gradient
    of the raw transpose `xt` is transposed back and added."""

    @staticmethod
    def forward(ctx, x_btc, want_raw, eps, input_bound):
        xn, xt = _instance_norm(x_btc, want_raw, eps, input_bound)
        ctx.eps = float(eps)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x_btc)
        return xn, xt

    @staticmethod
    def backward(ctx, gxn, gxt):
        x_btc, = ctx.saved_tensors
        gx = None
        if gxn is not None:
            _need_gpu("instance_norm backward", gxn)
            x = x_btc.contiguous()
            B, T, C = x.shape
            gxn = gxn.contiguous()
            gx = torch.empty_like(x)
            _lib.check(_lib.lib().ign_instnorm_bwd(_ptr(x), _ptr(gxn), _ptr(gx), B, T, C, ctx.eps, _stream()), "ign_instnorm_bwd")
        if gxt is not None:
            gt = gxt.permute(0, 2, 1)
            gx = gt.contiguous() if gx is None else gx + gt
        return gx, None, None, None


def contiguous_bct(x):
    """A contiguous (B, C, T) tensor with the contents of `x` (B, C, T).  If `x` is the `permute(0, 2, 1)` view of a contiguous
    time-first (B, T, C) batch -- what the harness hands the EEG-CNN baseline -- the transpose runs on ign_transpose_btc_to_bct
    (no gradient: input data); anything else takes torch's `.contiguous()`."""
    if x.is_contiguous():
        return x
    B, C, T = x.shape
    if (x.is_cuda and x.dtype == torch.float32 and not x.requires_grad and x.stride() == (T * C, 1, C) and B <= 65535
            and x.data_ptr() % 16 == 0):
        out = torch.empty(B, C, T, device=x.device, dtype=torch.float32)
        _lib.check(_lib.lib().ign_transpose_btc_to_bct(_ptr(x), _ptr(out), B, T, C, _stream()), "ign_transpose_btc_to_bct")
        return out
    return x.contiguous()


def standardise_nct_to_btc(x_nct, eps=1e-8):
    """Raw (B,C,T) recordings -> per-sample / per-channel standardised (B,T,C) batch on the GPU (the CHISCO loader's
    Normalizer('per_sample_std') + item transpose, IGN/data_factory/eeg.py:332-367, for the whole batch at once)."""
    _need_gpu("standardise_nct_to_btc", x_nct)
    x = x_nct.contiguous()
    B, C, T = x.shape
    out = torch.empty(B, T, C, device=x.device, dtype=torch.float32)
    ws = torch.empty(B * C * 2, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().ign_standardise_nct_to_btc(_ptr(x), _ptr(out), _ptr(ws), B, C, T, eps, _stream()),
               "ign_standardise_nct_to_btc")
    return out


EDGE_REFLECT, EDGE_ZERO = 0, 1       # IGN_EDGE_*


def _eeg_bank(name, x_nct, taps, quad, decimate, edge, channels, timepoints, eps):
    """The work eeg_filterbank and eeg_preprocess share, after their shape checks: taps (nb, M), quad (nb, M) or None."""
    if edge not in ("reflect", "zero"):
        raise ValueError(f"{name}: edge={edge!r} is neither 'reflect' nor 'zero'")
    x, h = x_nct.contiguous(), taps.contiguous()
    g = None if quad is None else quad.contiguous()
    B, Cin, Tin = x.shape
    nb, M = h.shape
    q = int(decimate)
    Td = -(-Tin // q) if q >= 1 else 0
    Cout = Cin if channels is None else int(channels)
    Tout = Td if timepoints is None else int(timepoints)
    L = _lib.lib()
    out = torch.empty(B, max(Tout, 0), max(nb * Cout, 0), device=x.device, dtype=torch.float32)
    ws = torch.empty(L.ign_eeg_filterbank_ws_bytes(B, Cin, Tin, M, nb, q, Cout, Tout) // 4 or 1, device=x.device, dtype=torch.float32)
    _lib.check(L.ign_eeg_filterbank_nct_to_btc(_ptr(x), _ptr(h), None if g is None else _ptr(g), _ptr(out), _ptr(ws), B, Cin, Tin, M,
                                               nb, q, EDGE_REFLECT if edge == "reflect" else EDGE_ZERO, Cout, Tout, eps, _stream()),
               "ign_eeg_filterbank_nct_to_btc")
    mask = (torch.arange(Tout, device=x.device) < min(Td, Tout)).unsqueeze(0).expand(B, Tout).contiguous()
    return out, mask


def eeg_preprocess(x_nct, taps, *, decimate=1, edge="reflect", channels=None, timepoints=None, eps=1e-8):
    """Raw (B,Cin,Tin) recordings -> (out (B,Tout,Cout), mask (B,Tout) bool) on the GPU: eeg_filterbank for the one band `taps`
    (M,) -- the centred FIR filter `taps` (float32, on the GPU, odd length), every `decimate`-th output, channels cropped /
    zero-padded to `channels` (None: Cin), time to `timepoints` (None: Td = ceil(Tin / decimate)), then the per-sample,
    per-channel standardisation of standardise_nct_to_btc over the Tv = min(Td, Tout) valid steps.  mask[b, t] = t < Tv; the
    output is exactly zero where the mask is false and in padded channels.  `edge`: how the row is extended by
    (len(taps) - 1) / 2 samples, 'reflect' (numpy pad 'reflect') or 'zero'."""
    name = "eeg_preprocess"
    _need_gpu(name, x_nct, taps)
    if x_nct.dim() != 3 or taps.dim() != 1:
        raise _lib.IgnError(f"{name}: expected x (B,Cin,Tin) and taps (M,), got {tuple(x_nct.shape)} and {tuple(taps.shape)}")
    return _eeg_bank(name, x_nct, taps.unsqueeze(0), None, decimate, edge, channels, timepoints, eps)


def eeg_filterbank(x_nct, taps, quad=None, *, decimate=1, edge="reflect", channels=None, timepoints=None, eps=1e-8):
    """Raw (B,Cin,Tin) recordings -> (out (B,Tout,nb*Cout), mask (B,Tout) bool) on the GPU (ign_eeg_filterbank_nct_to_btc; the rule
    is restated in utils/eeg_filter.py:filterbank_numpy): the nb bands `taps` (nb, M) at once -- the extended row is staged once
    and every band runs over it.  The output is band-major: channel j * Cout + c is electrode c of band j, each band block cropped /
    zero-padded to `channels` electrodes on its own, and without `quad` block j is eeg_preprocess(x, taps[j], ...) bit for bit.
    With `quad` (nb, M), the quadrature taps of utils.eeg_filter.design_quadrature, every band's output is its envelope
    sqrt(a^2 + b^2) before the standardisation; that needs edge='reflect' and M > 1."""
    name = "eeg_filterbank"
    _need_gpu(name, x_nct, taps, quad)
    if x_nct.dim() != 3 or taps.dim() != 2:
        raise _lib.IgnError(f"{name}: expected x (B,Cin,Tin) and taps (nb,M), got {tuple(x_nct.shape)} and {tuple(taps.shape)}")
    if quad is not None and tuple(quad.shape) != tuple(taps.shape):
        raise _lib.IgnError(f"{name}: quad {tuple(quad.shape)} does not have the shape of taps {tuple(taps.shape)}")
    return _eeg_bank(name, x_nct, taps, quad, decimate, edge, channels, timepoints, eps)


def _group_ids(name, gid, B):
    """The per-sample group ids as the spatial kernels take them: None, or a contiguous int32 (B) tensor on the GPU."""
    if gid is None:
        return None
    if not torch.is_tensor(gid) or not gid.is_cuda or gid.dtype != torch.int32 or tuple(gid.shape) != (B,):
        what = f"{gid.dtype} {tuple(gid.shape)} on {gid.device}" if torch.is_tensor(gid) else type(gid).__name__
        raise _lib.IgnError(f"{name}: gid must be an int32 tensor of shape ({B},) on the GPU, got {what}")
    return gid.contiguous()


def _spatial_out(name, out, shape, dtype, device):
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    if not out.is_cuda or out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise _lib.IgnError(f"{name}: out must be a contiguous {dtype} tensor of shape {tuple(shape)} on the GPU, got {out.dtype} "
                            f"{tuple(out.shape)} on {out.device}")
    return out


def eeg_spatial(x_nct, W, gid=None, *, out=None):
    """Raw (B,Cin,T) recordings -> y (B,Cs,T) on the GPU, y[b] = W[gid[b]] . x[b] across the electrodes (ign_eeg_spatial_nct; the
    rule, pivot included, is restated in utils/eeg_spatial.py:spatial_numpy): W (G,Cs,Cin) float32 on the GPU, a 2-D (Cs,Cin) W is
    one group; gid (B,) int32 on the GPU, None = group 0.  A gid outside [0,G) gives zeros for that sample.  The output keeps the
    input's layout, so standardise_nct_to_btc / eeg_filterbank run on it unchanged.  `out`: write into this tensor instead of a
    new one.  A non-contiguous x or W is copied."""
    name = "eeg_spatial"
    _need_gpu(name, x_nct, W)
    if x_nct.dim() != 3 or W.dim() not in (2, 3):
        raise _lib.IgnError(f"{name}: expected x (B,Cin,T) and W (G,Cs,Cin) or (Cs,Cin), got {tuple(x_nct.shape)} and {tuple(W.shape)}")
    w = (W.unsqueeze(0) if W.dim() == 2 else W).contiguous()
    x = x_nct.contiguous()
    B, Cin, T = x.shape
    G, Cs, Cw = w.shape
    if Cw != Cin:
        raise _lib.IgnError(f"{name}: W {tuple(W.shape)} takes {Cw} input channels, x {tuple(x_nct.shape)} has {Cin}")
    gid = _group_ids(name, gid, B)
    y = _spatial_out(name, out, (B, Cs, T), torch.float32, x.device)
    _lib.check(_lib.lib().ign_eeg_spatial_nct(_ptr(x), _ptr(w), _ptr(gid), _ptr(y), B, Cin, T, Cs, G, _stream()), "ign_eeg_spatial_nct")
    return y


def eeg_gram(x_nct, gid=None, groups=1, *, out=None):
    """(B,C,T) float32 on the GPU -> (gram (G,C,C) float32, count (G,) int32), G = `groups` (ign_eeg_gram_nct; restated in
    utils/eeg_spatial.py:gram_numpy): per group, the sum over its samples in ascending b of z z^T with z the rows minus their first
    sample, minus the mean of that.  Both outputs are overwritten -- zeros for an empty group -- and gram[g] is symmetric bit for
    bit; the caller accumulates batches (in float64).  `out`: (gram, count) tensors to write into."""
    name = "eeg_gram"
    _need_gpu(name, x_nct)
    if x_nct.dim() != 3:
        raise _lib.IgnError(f"{name}: expected x (B,C,T), got {tuple(x_nct.shape)}")
    x = x_nct.contiguous()
    B, C, T = x.shape
    G = int(groups)
    gid = _group_ids(name, gid, B)
    gram, count = (None, None) if out is None else out
    gram = _spatial_out(name, gram, (max(G, 0), C, C), torch.float32, x.device)
    count = _spatial_out(name, count, (max(G, 0),), torch.int32, x.device)
    L = _lib.lib()
    ws = torch.empty(L.ign_eeg_gram_ws_bytes(B, C, T, G) // 4 or 1, device=x.device, dtype=torch.float32)
    _lib.check(L.ign_eeg_gram_nct(_ptr(x), _ptr(gid), _ptr(gram), _ptr(count), _ptr(ws), B, C, T, G, _stream()), "ign_eeg_gram_nct")
    return gram, count


IIR_TABLE_COLUMNS = 8     # b0 b1 b2 a1 a2 zi1 zi2 0: one row of the section table ign_eeg_iir_nct reads


def eeg_iir(x_nct, coef, *, pad, g0, out=None):
    """Raw (B,C,T) recordings -> (B,C,T) float32 on the GPU, every row filtered forward and backward along time by a cascade of
    second-order sections (ign_eeg_iir_nct; the rule, in float64, is utils/eeg_iir.py:iir_numpy -- scipy's sosfiltfilt with an odd
    extension of `pad` samples): coef (ns,8) FLOAT64 on the GPU, rows (b0, b1, b2, a1, a2, zi1, zi2, 0), and g0 the squared DC gain,
    both from utils.eeg_iir.section_table.  The recurrence runs in float64 on the device; only the output is rounded.  The output
    keeps the input's layout, so standardise_nct_to_btc / eeg_filterbank run on it unchanged.  `out`: write into this tensor instead
    of a new one.  A non-contiguous x is copied.  Nothing of the call is a host value that a graph replay would freeze."""
    name = "eeg_iir"
    _need_gpu(name, x_nct)
    if not torch.is_tensor(coef) or not coef.is_cuda or coef.dtype != torch.float64 or coef.dim() != 2 or coef.shape[1] != IIR_TABLE_COLUMNS:
        what = f"{coef.dtype} {tuple(coef.shape)} on {coef.device}" if torch.is_tensor(coef) else type(coef).__name__
        raise _lib.IgnError(f"{name}: coef must be a float64 tensor of shape (ns,8) on the GPU, got {what}")
    if x_nct.dim() != 3:
        raise _lib.IgnError(f"{name}: expected x (B,C,T), got {tuple(x_nct.shape)}")
    x, table = x_nct.contiguous(), coef.contiguous()
    B, C, T = x.shape
    y = _spatial_out(name, out, (B, C, T), torch.float32, x.device)
    _lib.check(_lib.lib().ign_eeg_iir_nct(_ptr(x), _ptr(table), _ptr(y), B, C, T, int(table.shape[0]), int(pad), float(g0),
                                          _stream()), "ign_eeg_iir_nct")
    return y


def eeg_resample(x_nct, tab, *, up, down, half_len, edge="reflect", out=None):
    """Raw (B,C,Tin) recordings -> (B,C,Tout) float32 on the GPU, Tout = ceil(Tin * up / down): every row resampled by the ratio
    up/down (lowest terms) through the polyphase low-pass `tab` (ign_eeg_resample_nct; the rule, in float64, is
    utils/eeg_resample.py:resample_numpy -- scipy's resample_poly on the row minus its first sample, which is added back with gain
    exactly 1 so that the recording's offset never meets the phases' unequal DC gains).  tab (up,Lp) float32 on the GPU from
    utils.eeg_resample.phase_table, `half_len` the hl of its 2 hl + 1 taps; `edge`: how the row is extended by Lp samples, 'reflect'
    (numpy pad 'reflect') or 'zero'.  The output keeps the input's layout, so standardise_nct_to_btc / eeg_filterbank run on it
    unchanged.  `out`: write into this tensor instead of a new one.  A non-contiguous x is copied."""
    name = "eeg_resample"
    _need_gpu(name, x_nct, tab)
    if edge not in ("reflect", "zero"):
        raise _lib.IgnError(f"{name}: edge={edge!r} is neither 'reflect' nor 'zero'")
    if x_nct.dim() != 3 or tab.dim() != 2:
        raise _lib.IgnError(f"{name}: expected x (B,C,Tin) and tab (up,Lp), got {tuple(x_nct.shape)} and {tuple(tab.shape)}")
    up, down, hl = int(up), int(down), int(half_len)
    if up < 1 or down < 1:
        raise _lib.IgnError(f"{name}: up/down = {up}/{down} is not a positive ratio")
    if tab.shape[0] != up:
        raise _lib.IgnError(f"{name}: tab {tuple(tab.shape)} does not hold up={up} phases")
    x, table = x_nct.contiguous(), tab.contiguous()
    B, C, Tin = x.shape
    Tout = -(-Tin * up // down)
    y = _spatial_out(name, out, (B, C, Tout), torch.float32, x.device)
    _lib.check(_lib.lib().ign_eeg_resample_nct(_ptr(x), _ptr(table), _ptr(y), B, C, Tin, Tout, up, down, hl, int(table.shape[1]),
                                               EDGE_REFLECT if edge == "reflect" else EDGE_ZERO, _stream()), "ign_eeg_resample_nct")
    return y


def _artifact_weights(name, w, C):
    """The neighbour weights as ign_eeg_artifact_apply_nct takes them: None, or a contiguous float32 (C,C) tensor on the GPU without
    a negative or non-finite entry.  The kernel trusts the values, so they are checked here, on the host, once per tensor."""
    if w is None:
        return None
    if not torch.is_tensor(w) or not w.is_cuda or w.dtype != torch.float32 or tuple(w.shape) != (C, C):
        what = f"{w.dtype} {tuple(w.shape)} on {w.device}" if torch.is_tensor(w) else type(w).__name__
        raise _lib.IgnError(f"{name}: neighbors must be a float32 tensor of shape ({C},{C}) on the GPU, got {what}")
    w = w.contiguous()
    if getattr(w, "_ign_artifact_checked", None) != w._version:
        if not bool((torch.isfinite(w) & (w >= 0)).all()):
            raise _lib.IgnError(f"{name}: neighbors holds a negative or non-finite weight")
        w._ign_artifact_checked = w._version
    return w


def eeg_artifact(x_nct, clip=None, flat=None, noisy=None, neighbors=None, out=None):
    """Raw (B,C,T) recordings -> (out (B,C,T) float32, verdict (B,C) uint8, stats (B,C,2) float32) on the GPU
    (ign_eeg_artifact_stats_nct + ign_eeg_artifact_apply_nct; the rule is utils/eeg_artifact.py:artifact_numpy): per row the lower
    median m and the median absolute deviation s; per electrode a verdict 0 good, 1 flat (s <= flat * ref), 2 noisy
    (s > noisy * ref), 3 non-finite, 4 unrepaired, ref the lower median of s over the sample's finite rows; good rows clamped to
    m +- clip * 1.4826 * s; bad rows rebuilt as the `neighbors`-weighted mean of the centred good rows.  None switches a key off
    (flat=0: only s = 0 is flat); `neighbors`: (C,C) float32 non-negative on the GPU, None = all ones.  Statistics, verdicts and good
    rows are bit for bit the numpy rule.  `out`: the out tensor, or (out, verdict, stats), to write into.  A non-contiguous x is
    copied.  Three launches, no host synchronisation (the weights are checked once per tensor)."""
    name = "eeg_artifact"
    _need_gpu(name, x_nct)
    if x_nct.dim() != 3:
        raise _lib.IgnError(f"{name}: expected x (B,C,T), got {tuple(x_nct.shape)}")
    from utils.eeg_artifact import kernel_keys
    k, f, n = (float(v) for v in kernel_keys(clip, flat, noisy))
    x = x_nct.contiguous()
    B, C, T = x.shape
    w = _artifact_weights(name, neighbors, C)
    y, verdict, stats = out if isinstance(out, (tuple, list)) else (out, None, None)
    y = _spatial_out(name, y, (B, C, T), torch.float32, x.device)
    verdict = _spatial_out(name, verdict, (B, C), torch.uint8, x.device)
    stats = _spatial_out(name, stats, (B, C, 2), torch.float32, x.device)
    flags = torch.empty(B, C, device=x.device, dtype=torch.uint8)
    L = _lib.lib()
    _lib.check(L.ign_eeg_artifact_stats_nct(_ptr(x), _ptr(stats), _ptr(flags), B, C, T, _stream()), "ign_eeg_artifact_stats_nct")
    _lib.check(L.ign_eeg_artifact_apply_nct(_ptr(x), _ptr(stats), _ptr(flags), _ptr(w), _ptr(y), _ptr(verdict), B, C, T, k, f, n,
                                            _stream()), "ign_eeg_artifact_apply_nct")
    return y, verdict, stats


_UNSEEDED = object()


def _batch_transform(name, acts, x, lengths, check, seed=_UNSEEDED, more=()):
    """The shared opening of ops.augment / ops.warp / ops.mix, in the order in which each of them refuses: fp32 on the GPU (`x` and
    `more`), a contiguous (B,T,C) batch without a gradient, for a seeded op no graph capture, then the op's own `check()`; ->
    (out, lengths, seed): a new tensor like `x`, and for B > 0 the checked lengths and the seed as 64 bits.  B == 0: nothing to launch."""
    _need_gpu(name, x, *more)
    if x.dim() != 3 or not x.is_contiguous():
        raise _lib.IgnError(f"{name}: expected a contiguous (B,T,C) tensor, got shape {tuple(x.shape)} strides {x.stride()}")
    if x.requires_grad:
        raise _lib.IgnError(f"{name}: the input requires a gradient; {acts} acts on data (there is no backward pass)")
    if seed is not _UNSEEDED and torch.cuda.is_current_stream_capturing():
        raise _lib.IgnError(f"{name} inside a hipGraph capture: the per-call seed would be frozen into the graph ({name} the batch "
                            f"before the captured step)")
    check()
    out = torch.empty_like(x)
    if x.shape[0]:
        lengths = None if lengths is None else _lengths(name, lengths, x.shape[0])
        seed = None if seed is _UNSEEDED else int(seed) & 0xFFFFFFFFFFFFFFFF
    return out, lengths, seed


def augment(x, seed, *, lengths=None, shift=0.0, scale=0.0, noise=0.0, channel_drop=0.0, time_mask=0.0):
    """Training augmentation of a contiguous fp32 (B,T,C) batch on the GPU -> a new tensor (ign_augment_btc; the rule is
    csrc/ign_augment.h, restated in utils/augment.py): a circular shift by up to `shift` * length, a per-channel gain in
    1 +- `scale`, Gaussian noise of standard deviation `noise`, electrode dropout at rate `channel_drop` (no rescaling) and one
    masked time span of up to `time_mask` * length per sample.  `lengths`: int32 (B,) on the GPU -- everything happens inside each
    sample's own length and the padding is copied through; None: every sample has T steps.  `seed`: a 64-bit host integer; the
    same seed gives the same output to the bit.  Rates lie in [0, 1), `noise` >= 0.
    Refused for an input that requires a gradient (a training batch never does) and during graph capture (the seed is a host
    value: a replay would repeat one augmentation)."""
    name = "augment"

    def check():
        for what, v in (("shift", shift), ("scale", scale), ("time_mask", time_mask)):
            if not 0.0 <= ctypes.c_float(v).value < 1.0:
                raise ValueError(f"{name}: {what} = {v} outside [0, 1)")
        if not 0.0 <= ctypes.c_float(noise).value < float("inf"):
            raise ValueError(f"{name}: noise = {noise} must be finite and >= 0")
        try:
            dropout_threshold(channel_drop)                        # the keep rule of attention dropout: halfword >= round(p * 65536)
        except ValueError:
            raise ValueError(f"{name}: channel_drop = {channel_drop} outside [0, 1)") from None
    out, lengths, seed = _batch_transform(name, "augmentation", x, lengths, check, seed)
    B, T, C = x.shape
    if B:
        _lib.check(_lib.lib().ign_augment_btc(_ptr(x), _ptr(out), _ptr(lengths), B, T, C, seed, shift, scale, noise,
                                              dropout_threshold(channel_drop)[0], time_mask, _stream()), "ign_augment_btc")
    return out


def warp(x, seed, lengths=None, twarp=0.0, mwarp=0.0, wwarp=0.0, knots=4, prob=1.0):
    """Time, magnitude and window warping of a contiguous fp32 (B,T,C) batch on the GPU -> a new tensor (ign_warp_btc; the rule is
    csrc/ign_warp.h, restated in utils/warp.py): every sample is resampled along time through its own monotone map -- a smooth
    speed curve through `knots` interior knots in 1 +- `twarp`, and one window of `wwarp` * length stretched or compressed by 2 -- and
    scaled by a smooth gain curve in 1 +- `mwarp` shared by its channels; a sample is warped with probability `prob`, else copied.
    `lengths`: int32 (B,) on the GPU -- everything happens inside each sample's own length and the padding is copied through;
    None: every sample has T steps.  `seed`: a 64-bit host integer; the same seed gives the same output to the bit.  Rates lie in
    [0, 1), knots in 1..8, prob in (0, 1].  One launch, also when every rate is 0 (a copy).
    Refused for an input that requires a gradient (a training batch never does) and during graph capture (the seed is a host
    value: a replay would repeat one warp)."""
    name = "warp"
    from utils.warp import check_spec
    out, lengths, seed = _batch_transform(name, "warping", x, lengths, lambda: check_spec(twarp, mwarp, wwarp, knots, prob, who=name),
                                          seed)
    B, T, C = x.shape
    if B:
        _lib.check(_lib.lib().ign_warp_btc(_ptr(x), _ptr(out), _ptr(lengths), B, T, C, seed, twarp, mwarp, wwarp, int(knots), prob,
                                           _stream()), "ign_warp_btc")
    return out


def mix(x, lam, roll, span=None, lengths=None):
    """Mixup / CutMix of a contiguous fp32 (B,T,C) batch on the GPU -> a new tensor (ign_mix_btc; the rule is restated in
    utils/mix.py:mix_reference): sample b is blended with its partner p = (b + roll) mod B as lam[b] * x[b] + (1 - lam[b]) * x[p],
    replaced by the partner inside its span (start, m) = span[b], and left as it is from lengths[b] on and where lam[b] == 1.
    `lam`: float32 (B,), `span`: int32 (B, 2) or None (no spans), `lengths`: int32 (B,) or None (every sample has T steps), all on
    the GPU; `roll`: a host integer in [0, B).  The draws come from utils.mix.mix_draws.  Refused for an input that requires a
    gradient (a training batch never does).  Every argument but `roll` is device data, so the call may be captured."""
    name = "mix"

    def check():
        B = x.shape[0]
        if tuple(lam.shape) != (B,):
            raise _lib.IgnError(f"{name}: lam must be a float32 tensor of shape ({B},), got {tuple(lam.shape)}")
        if span is not None and not (torch.is_tensor(span) and span.is_cuda and span.dtype == torch.int32 and tuple(span.shape) == (B, 2)):
            what = f"{span.dtype} {tuple(span.shape)} on {span.device}" if torch.is_tensor(span) else type(span).__name__
            raise _lib.IgnError(f"{name}: span must be an int32 tensor of shape ({B}, 2) on the GPU, got {what}")
        if not 0 <= int(roll) < max(B, 1):
            raise _lib.IgnError(f"{name}: roll = {int(roll)} outside [0, {B})")
    out, lengths, _ = _batch_transform(name, "mixing", x, lengths, check, more=(lam,))
    B, T, C = x.shape
    if B:
        _lib.check(_lib.lib().ign_mix_btc(_ptr(x), _ptr(out), _ptr(lengths), _ptr(lam.contiguous()),
                                          _ptr(None if span is None else span.contiguous()), int(roll), B, T, C, _stream()),
                   "ign_mix_btc")
    return out


def _tables(G):
    return ctypes.c_void_p * G, ctypes.c_int * G


def _pv(ts):
    return (ctypes.c_void_p * len(ts))(*[(t.data_ptr() if t is not None else None) for t in ts])


BANK_MAX_GROUPS = 8           # SHP_MAX_GROUPS (csrc/ign_common.h): most groups one ign_shapelet_*_bank call takes

# one length group of a bank: parameters, window geometry, first column in P / D, and what the forward saves for the backward
_Group = namedtuple("_Group", "w thr K L stride Tw col0 tstar zmu dsave xstat")


class _Bank:
    """Host record of one bank forward, built once and kept on the autograd node: the groups, the shape (B, C, T), ld = sum_g K_g*C
    (the row length of P / D, feature order g*K*C + k*C + c as IGN/model/Shapelet.py:84,195-196), eps, mode, and the host tables the
    ign_shapelet_*_bank entry points read -- shared by the three launchers below."""

    def __init__(self, xn, ws, thrs, eps, mode, strides, need_grad):
        B, C, T = xn.shape
        self.B, self.C, self.T, self.eps, self.mode, self.need_grad = B, C, T, float(eps), int(mode), need_grad
        f32 = dict(device=xn.device, dtype=torch.float32)
        want_xstat = need_grad and (mode & 0xf) >= DIST_COS
        self.groups, col0 = [], 0
        for g, (w, thr) in enumerate(zip(ws, thrs)):
            K, Cw, Lg = w.shape
            if Cw != C:
                raise _lib.IgnError(f"shapelet group {g}: weights have {Cw} channels, input has {C}")
            stride = int(strides[g])
            Tw = (T - Lg) // stride + 1
            self.groups.append(_Group(
                w=w, thr=thr, K=K, L=Lg, stride=stride, Tw=Tw, col0=col0,
                tstar=torch.empty(B, K, C, device=xn.device, dtype=torch.int32), zmu=torch.empty(B, K, C, 2, **f32),
                dsave=torch.empty(B, C, K, Tw, **f32) if need_grad else None, xstat=torch.empty(B, C, Tw, **f32) if want_xstat else None))
            col0 += K * C
        self.G, self.ld, self.n_thr = len(self.groups), col0, (len(self.groups) if mode & GATE_LTS else 0)
        self.one_call = self.G <= BANK_MAX_GROUPS     # the *_bank entry points take the whole bank; else: group by group
        cols = {f: [getattr(s, f) for s in self.groups] for f in _Group._fields}
        self.Ks, self.Ls, self.Ss, self.col0s = ((ctypes.c_int * self.G)(*cols[f]) for f in ("K", "L", "stride", "col0"))
        self.ws, self.thrs, self.tstars, self.zmus, self.dsaves, self.xstats = (
            _pv(cols[f]) for f in ("w", "thr", "tstar", "zmu", "dsave", "xstat"))

    def cat_tstar(self):
        ts = [s.tstar.reshape(self.B, -1) for s in self.groups]
        return torch.cat(ts, dim=1) if len(ts) > 1 else ts[0]


def _bank_fwd(bank, xn):
    """Forward of every length group: -> (P, D), both (B, ld); the arg-max windows, statistics and distances land in `bank`."""
    P = torch.empty(bank.B, bank.ld, device=xn.device, dtype=torch.float32)
    D = torch.empty_like(P)
    L = _lib.lib()
    if bank.one_call:          # (ign_shapelet_fwd_bank validates every group, then launches group by group)
        _lib.check(L.ign_shapelet_fwd_bank(
            _ptr(xn), bank.G, bank.ws, bank.thrs, _ptr(P), _ptr(D), bank.ld, bank.col0s, bank.tstars, bank.zmus, bank.dsaves, bank.xstats,
            bank.B, bank.C, bank.T, bank.Ks, bank.Ls, bank.Ss, bank.eps, bank.mode, _stream()), "ign_shapelet_fwd_bank")
    else:
        for s in bank.groups:
            _lib.check(L.ign_shapelet_fwd(
                _ptr(xn), _ptr(s.w), _ptr(s.thr), _ptr(P), _ptr(D), bank.ld, s.col0, _ptr(s.tstar), _ptr(s.zmu), _ptr(s.dsave),
                _ptr(s.xstat), bank.B, bank.C, bank.T, s.K, s.L, s.stride, bank.eps, bank.mode, _stream()), "ign_shapelet_fwd")
    return P, D


def _bank_regate(bank, lengths, P, D):
    """The length-aware pass behind _bank_fwd (ign_shapelet_regate): P, D and the record's arg-max windows, statistics and saved
    distances become those of every sample truncated to lengths[b], in place."""
    L = _lib.lib()
    if bank.one_call:
        _lib.check(L.ign_shapelet_regate_bank(
            bank.G, bank.dsaves, _ptr(lengths), bank.thrs, _ptr(P), _ptr(D), bank.ld, bank.col0s, bank.tstars, bank.zmus,
            bank.B, bank.C, bank.T, bank.Ks, bank.Ls, bank.Ss, bank.eps, bank.mode, _stream()), "ign_shapelet_regate_bank")
    else:
        for s in bank.groups:
            _lib.check(L.ign_shapelet_regate(
                _ptr(s.dsave), _ptr(lengths), _ptr(s.thr), _ptr(P), _ptr(D), bank.ld, s.col0, _ptr(s.tstar), _ptr(s.zmu),
                bank.B, bank.C, bank.T, s.K, s.L, s.stride, bank.eps, bank.mode, _stream()), "ign_shapelet_regate")


def _bank_wgrad(bank, xn, gP, P, D, gw_add=None, add_scale=None):
    """dloss/dw of every group (list of (K,C,L) tensors) from gP = dloss/dP (B, ld).  `gw_add[g]` / `add_scale` (a one-element
    device tensor): a batch-independent gradient of the same shapelets that the reduction launch adds as add_scale * gw_add[g]
    (the diversity regulariser) -- a parameter with two gradient sources then needs no accumulate kernel (group by group: torch)."""
    B, C, T, mode = bank.B, bank.C, bank.T, bank.mode
    L = _lib.lib()
    cos = (mode & 0xf) >= DIST_COS
    wnorms = [s.w.square().sum(dim=-1).sqrt().contiguous() if cos else None for s in bank.groups]
    gws = [torch.empty_like(s.w) for s in bank.groups]
    if bank.one_call:
        Ks, Ls, Ss = bank.Ks, bank.Ls, bank.Ss
        nbytes = L.ign_shapelet_bwd_bank_workspace_bytes(bank.G, B, C, T, Ks, Ls, Ss, mode)
        if nbytes == 0:
            raise _lib.IgnError(f"shapelet backward: no launch plan for K={list(Ks)} L={list(Ls)} stride={list(Ss)}")
        work = torch.empty(nbytes // 4, device=xn.device, dtype=torch.float32)
        _lib.check(L.ign_shapelet_bwd_bank(
            _ptr(xn), bank.G, bank.ws, _ptr(gP), _ptr(P), _ptr(D), bank.ld, bank.col0s, bank.tstars, bank.zmus, bank.dsaves, bank.xstats,
            _pv(wnorms), _pv(gws), _pv(gw_add) if gw_add is not None else None, _ptr(add_scale), _ptr(work), B, C, T, Ks, Ls, Ss,
            bank.eps, mode, _stream()), "ign_shapelet_bwd_bank")
        return gws
    for g, s in enumerate(bank.groups):
        nbytes = L.ign_shapelet_bwd_workspace_bytes(B, C, T, s.K, s.L, s.stride, mode)
        if nbytes == 0:
            raise _lib.IgnError(f"shapelet backward: no launch plan for K={s.K} L={s.L} stride={s.stride}")
        work = torch.empty(nbytes // 4, device=xn.device, dtype=torch.float32)
        _lib.check(L.ign_shapelet_bwd(
            _ptr(xn), _ptr(s.w), _ptr(gP), _ptr(P), _ptr(D), bank.ld, s.col0, _ptr(s.tstar), _ptr(s.zmu), _ptr(s.dsave), _ptr(s.xstat),
            _ptr(wnorms[g]), _ptr(gws[g]), _ptr(work), B, C, T, s.K, s.L, s.stride, bank.eps, mode, _stream()), "ign_shapelet_bwd")
        if gw_add is not None and gw_add[g] is not None:
            gws[g] = gws[g] + (gw_add[g] if add_scale is None else gw_add[g] * add_scale)
    return gws


def _bank_xgrad(bank, xn, gP, P, D):
    """dloss/dxn (B,C,T) of every group from gP = dloss/dP (B, ld): the groups run one after another on the stream, the first
    overwriting the result and the others adding to it (no atomics: bitwise repeatable)."""
    L = _lib.lib()
    gxn = torch.empty_like(xn)
    if bank.one_call:
        _lib.check(L.ign_shapelet_bwd_input_bank(
            _ptr(xn), bank.G, bank.ws, _ptr(gP), _ptr(P), _ptr(D), bank.ld, bank.col0s, bank.tstars, bank.zmus, bank.dsaves, _ptr(gxn),
            bank.B, bank.C, bank.T, bank.Ks, bank.Ls, bank.Ss, bank.eps, bank.mode, _stream()), "ign_shapelet_bwd_input_bank")
    else:
        for g, s in enumerate(bank.groups):
            _lib.check(L.ign_shapelet_bwd_input(
                _ptr(xn), _ptr(s.w), _ptr(gP), _ptr(P), _ptr(D), bank.ld, s.col0, _ptr(s.tstar), _ptr(s.zmu), _ptr(s.dsave), _ptr(gxn),
                1 if g else 0, bank.B, bank.C, bank.T, s.K, s.L, s.stride, bank.eps, bank.mode, _stream()), "ign_shapelet_bwd_input")
    return gxn


def _input_grad_supported(name, mode):
    """Raise at FORWARD time when the input needs a gradient the kernels do not produce (cosine / pearson)."""
    if (mode & 0xf) >= DIST_COS:
        raise _lib.IgnError(f"{name}: the input requires a gradient, but input gradients through the shapelet bank exist for the "
                            f"L1 ('euclidean') and MSE (memory_efficient) distances only, not for cosine / pearson (mode 0x{mode:x})")


def _threshold_grads(bank, gP, P):
    """LTS: dP/dthr = sigma'(thr - m) = P(1-P), summed over the batch  (IGN/model/Shapelet.py:109)"""
    gt = (gP * P * (1 - P)).sum(0)
    return [gt[s.col0:s.col0 + s.K * bank.C].view(1, s.K, bank.C) for s in bank.groups]


def _node_forward(xn, others, params, G, eps, mode, strides, need_x, need_rest, gpu_name, grad_name, lengths=None):
    """What the forwards of ShapeletBankFn and SbmFn share: unpack w_0..w_{G-1}[, thr_0..thr_{G-1}], refuse what the kernels do not
    take (`gpu_name` / `grad_name`: the node in a device / dtype error / in the input-gradient refusal; `others`: its further tensor inputs), build
    the record and run the forward -> (xn, bank, P, D).  The distances are kept when the input alone needs a gradient.
    `lengths` (ShapeletBankLenFn): the record always keeps the distances, and the regate pass runs behind the forward."""
    ws = [w.contiguous() for w in params[:G]]
    thrs = [t.contiguous() for t in params[G:]] if (mode & GATE_LTS) else [None] * G
    _need_gpu(gpu_name, xn, *others, *ws, *[t for t in thrs if t is not None])
    xn = xn.contiguous()
    if need_x:
        _input_grad_supported(grad_name, mode)
    if lengths is None:
        bank = _Bank(xn, ws, thrs, eps, mode, strides, need_x or need_rest)
        return (xn, bank, *_bank_fwd(bank, xn))
    lengths = _lengths(gpu_name, lengths, xn.shape[0])
    bank = _Bank(xn, ws, thrs, eps, mode, strides, True)
    P, D = _bank_fwd(bank, xn)
    _bank_regate(bank, lengths, P, D)
    return xn, bank, P, D


def _node_backward(bank, xn, gP, P, D, need_x, need_params, gw_add=None, add_scale=None):
    """What the backwards share, from gP = dloss/dP (None: nothing reached P): -> (gxn, grads_w, grads_t), the lists with one entry
    per group / per threshold (none without LTS).  Only the input needing a gradient means no weight / threshold work."""
    none = [None] * bank.G, [None] * bank.n_thr
    if gP is None:
        return (None, *none)
    gP = gP.contiguous()
    gxn = _bank_xgrad(bank, xn, gP, P, D) if need_x else None
    if need_x and not need_params:
        return (gxn, *none)
    return gxn, _bank_wgrad(bank, xn, gP, P, D, gw_add, add_scale), (_threshold_grads(bank, gP, P) if bank.n_thr else [])


class ShapeletBankFn(torch.autograd.Function):
    """All length groups of a shapelet bank in one autograd node.

    forward(xn, eps, mode, stride_list, n_groups, w_0..w_{G-1}[, thr_0..thr_{G-1}]) -> (P, Dmin, Tstar), all
    (B, sum_g K_g*C) with the reference's feature order g*K*C + k*C + c (IGN/model/Shapelet.py:84,195-196).
    Dmin is non-differentiable (the training loss never reads it: IGN/exp/experiment_classification.py:325-329).
    Tstar (int32) is the WINDOW INDEX of the best match -- arg-max_t p for the RBF gate, arg-min_t d for LTS, first index on
    ties; the match covers samples [Tstar*stride, Tstar*stride + L) -- which is what the reference's shapelet plots need
    (IGN/utils/shapelet_util.py:153 recomputes it on the host by sliding every shapelet over every series).
    The node keeps the bank record (`ctx.bank`, a _Bank); xn, P, Dmin and the parameters go through save_for_backward.
    """

    @staticmethod
    def forward(ctx, xn, eps, mode, strides, n_groups, *params):
        xn, bank, P, D = _node_forward(xn, (), params, n_groups, eps, mode, strides, ctx.needs_input_grad[0],
                                       any(ctx.needs_input_grad[5:]), gpu_name="shapelet_fwd", grad_name="shapelet_bank")
        Tstar = bank.cat_tstar()
        ctx.mark_non_differentiable(D, Tstar)
        ctx.set_materialize_grads(False)              # (else autograd fills a zero tensor per unused output, one launch each)
        ctx.bank = bank
        ctx.save_for_backward(xn, P, D, *(s.w for s in bank.groups), *(s.thr for s in bank.groups if s.thr is not None))
        return P, D, Tstar

    @staticmethod
    def backward(ctx, gP, gD, gT):
        if not ctx.bank.need_grad:
            raise _lib.IgnError("shapelet backward called but the forward ran without saving distances")
        xn, P, D = ctx.saved_tensors[:3]
        gxn, grads_w, grads_t = _node_backward(ctx.bank, xn, gP, P, D, ctx.needs_input_grad[0], any(ctx.needs_input_grad[5:]))
        return (gxn, None, None, None, None, *grads_w, *grads_t)


class ShapeletBankLenFn(torch.autograd.Function):
    """ShapeletBankFn for a batch zero-padded at the end, `xn` from instance_norm_len with the same `lengths`: every sample is
    matched as if it had been given alone, truncated to lengths[b] -- group g sees its first Tw_b = (n_b - L_g) // stride_g + 1
    windows.  forward(xn, lengths, eps, mode, stride_list, n_groups, w_0..[, thr_0..]) -> (P, Dmin, Tstar); a feature without a
    window (n_b < L_g) has P = 0, Dmin = NO_WINDOW, Tstar = -1 and neither receives nor sends a gradient.  The same forward and
    backward kernels: the regate pass (_bank_regate) rewrites what the forward saved, so what autograd keeps (P, Dmin, the record)
    is the regated state and the weight / threshold gradients are the sums of those of the truncated problems.  No input gradient."""

    @staticmethod
    def forward(ctx, xn, lengths, eps, mode, strides, n_groups, *params):
        _no_input_grad_with_lengths("shapelet_bank", ctx.needs_input_grad[0])
        xn, bank, P, D = _node_forward(xn, (), params, n_groups, eps, mode, strides, False, any(ctx.needs_input_grad[6:]),
                                       gpu_name="shapelet_fwd", grad_name="shapelet_bank", lengths=lengths)
        Tstar = bank.cat_tstar()
        ctx.mark_non_differentiable(D, Tstar)
        ctx.set_materialize_grads(False)
        ctx.bank = bank
        ctx.save_for_backward(xn, P, D, *(s.w for s in bank.groups), *(s.thr for s in bank.groups if s.thr is not None))
        return P, D, Tstar

    @staticmethod
    def backward(ctx, gP, gD, gT):
        xn, P, D = ctx.saved_tensors[:3]
        _, grads_w, grads_t = _node_backward(ctx.bank, xn, gP, P, D, False, True)
        return (None, None, None, None, None, None, *grads_w, *grads_t)


def shapelet_bank(xn, weights, eps, mode=DIST_L1 | GATE_RBF, strides=None, thresholds=None, return_tstar=False, lengths=None):
    """-> (P, Dmin) or, with return_tstar, (P, Dmin, Tstar): see ShapeletBankFn; with `lengths` (int32 (B) on the GPU; `xn` from
    instance_norm_len): ShapeletBankLenFn."""
    G = len(weights)
    if (mode & 0xf) == DIST_PEARSON:
        # pearson_corrcoef centres both operands (Shapelet.py:11-19).  <x - mean x, w_c> == <x, w_c> for a centred w_c,
        # so the kernel gets the centred shapelets and autograd projects the gradient back through this subtraction.
        weights = [w - w.mean(dim=-1, keepdim=True) for w in weights]
    strides = strides or [1] * G
    params = list(weights) + (list(thresholds) if (mode & GATE_LTS) else [])
    if lengths is None:
        P, D, Tstar = ShapeletBankFn.apply(xn, eps, mode, tuple(strides), G, *params)
    else:
        P, D, Tstar = ShapeletBankLenFn.apply(xn, lengths, eps, mode, tuple(strides), G, *params)
    return (P, D, Tstar) if return_tstar else (P, D)


def _kmeans_stats(name, w, sums, counts, inertia):
    """Check the statistics tensors of a k-means step against the centroids w (K,C,L): sums (K,C,L) fp32, counts (K,C) int32,
    inertia (C) fp32, all contiguous on w's device."""
    K, C, L = w.shape
    _need_gpu(name, w, sums, inertia)
    if not counts.is_cuda or counts.dtype != torch.int32:
        raise _lib.IgnError(f"{name}: counts must be an int32 tensor on the GPU, got {counts.dtype} on {counts.device}")
    for label, t, shape in (("sums", sums, (K, C, L)), ("counts", counts, (K, C)), ("inertia", inertia, (C,))):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous()):
            raise _lib.IgnError(f"{name}: {label} must be a contiguous tensor of shape {shape}, got {tuple(t.shape)}")


def shapelet_kmeans_step(xn, w, stride=1, sums=None, counts=None, inertia=None, return_assign=False):
    """One Lloyd step of one length group over a batch (ign_shapelet_kmeans_step): every window xn[b, c, t*stride : t*stride+L]
    of the instance-normalised (B,C,T) batch goes to the nearest (mean squared difference, lowest k on ties) of the K centroids
    w[:, c, :] of its channel.  -> (sums (K,C,L), counts (K,C) int32, inertia (C))[, assign (B,C,Tw) int32]: the sum of the
    windows of each cluster, its size, and the summed minimum distances per channel.  sums / counts / inertia None: allocated and
    overwritten; given (all three): added to, for a training set streamed batch by batch.  Bitwise repeatable; no gradient."""
    name = "shapelet_kmeans_step"
    _need_gpu(name, xn, w)
    given = [t is not None for t in (sums, counts, inertia)]
    if any(given) and not all(given):
        raise _lib.IgnError(f"{name}: pass sums, counts and inertia together (accumulate) or none of them (overwrite)")
    if xn.dim() != 3 or w.dim() != 3 or w.shape[1] != xn.shape[1]:
        raise _lib.IgnError(f"{name}: xn must be (B,C,T) and w (K,C,L) with the same C, got {tuple(xn.shape)} and {tuple(w.shape)}")
    xn, wc = xn.detach().contiguous(), w.detach().contiguous()
    B, C, T = xn.shape
    K, _, Lw = wc.shape
    stride = int(stride)
    accumulate = all(given)
    if not accumulate:
        sums = torch.empty(K, C, Lw, device=xn.device, dtype=torch.float32)
        counts = torch.empty(K, C, device=xn.device, dtype=torch.int32)
        inertia = torch.empty(C, device=xn.device, dtype=torch.float32)
    _kmeans_stats(name, wc, sums, counts, inertia)
    L = _lib.lib()
    nbytes = L.ign_shapelet_kmeans_workspace_bytes(B, C, T, K, Lw, stride)
    work = torch.empty(max(nbytes, 4) // 4, device=xn.device, dtype=torch.int32)     # (0 bytes: the step call reports why)
    assign = None
    if return_assign and nbytes:
        assign = torch.empty(B, C, (T - Lw) // stride + 1, device=xn.device, dtype=torch.int32)
    _lib.check(L.ign_shapelet_kmeans_step(_ptr(xn), _ptr(wc), _ptr(assign), _ptr(sums), _ptr(counts), _ptr(inertia), _ptr(work),
                                          1 if accumulate else 0, B, C, T, K, Lw, stride, _stream()), "ign_shapelet_kmeans_step")
    return (sums, counts, inertia, assign) if return_assign else (sums, counts, inertia)


def shapelet_kmeans_update(w, sums, counts):
    """w[k,c,:] = sums[k,c,:] / counts[k,c] where counts > 0, in place and outside autograd (ign_shapelet_kmeans_update); an empty
    cluster keeps its centroid bit for bit.  Returns w."""
    name = "shapelet_kmeans_update"
    if w.dim() != 3 or not w.is_contiguous():
        raise _lib.IgnError(f"{name}: w must be a contiguous (K,C,L) tensor (it is written in place), got {tuple(w.shape)}")
    _kmeans_stats(name, w, sums, counts, None)
    K, C, Lw = w.shape
    with torch.no_grad():
        _lib.check(_lib.lib().ign_shapelet_kmeans_update(_ptr(w), _ptr(sums), _ptr(counts), K, C, Lw, _stream()),
                   "ign_shapelet_kmeans_update")
        _lib.PARAM_GENERATION[0] += 1        # parameter values changed behind autograd's back (see _lib.PARAM_GENERATION)
    return w


def _project_inputs(name, xn, d, t):
    """The batch-side tensors of a projection step: xn (B,C,T) fp32, d (B,ld) fp32 and t (B,ld) int32 -- the Dmin and Tstar of
    shapelet_bank(..., return_tstar=True) on that xn -- contiguous on the GPU."""
    _need_gpu(name, xn, d)
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.int32:
        what = f"{t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise _lib.IgnError(f"{name}: t must be an int32 tensor on the GPU, got {what}")
    if xn.dim() != 3 or d.dim() != 2 or d.shape[0] != xn.shape[0] or t.shape != d.shape:
        raise _lib.IgnError(f"{name}: xn must be (B,C,T) and d, t (B,ld) with the same B and ld, got {tuple(xn.shape)}, "
                            f"{tuple(d.shape)} and {tuple(t.shape)}")
    return xn.detach().contiguous(), d.detach().contiguous(), t.contiguous()


def _project_state(name, device, w_shape, state):
    """-> ((best_d (K,C) f32, best_src (K,C,2) i32, cand (K,C,L) f32), accumulate): allocated when `state` is None, checked else."""
    K, C, Lw = (int(v) for v in w_shape)
    if state is None:
        return (torch.empty(K, C, device=device, dtype=torch.float32), torch.empty(K, C, 2, device=device, dtype=torch.int32),
                torch.empty(K, C, Lw, device=device, dtype=torch.float32)), 0
    best_d, best_src, cand = state
    _need_gpu(name, best_d, cand)
    if not best_src.is_cuda or best_src.dtype != torch.int32:
        raise _lib.IgnError(f"{name}: best_src must be an int32 tensor on the GPU, got {best_src.dtype} on {best_src.device}")
    for label, s, shape in (("best_d", best_d, (K, C)), ("best_src", best_src, (K, C, 2)), ("cand", cand, (K, C, Lw))):
        if tuple(s.shape) != shape or not s.is_contiguous():
            raise _lib.IgnError(f"{name}: {label} must be a contiguous tensor of shape {shape}, got {tuple(s.shape)}")
    return (best_d, best_src, cand), 1


def shapelet_project_step(xn, d, t, col0, w_shape, stride, sample0, state=None):
    """One batch of the projection of one length group (ign_shapelet_project_step), behind the shapelet forward of that batch:
    `d`, `t` (B, ld) are the Dmin and Tstar of shapelet_bank(xn, ..., return_tstar=True), the group's features start at column
    `col0`, its shapelets have shape w_shape = (K, C, L) and window step `stride`; `sample0` is the ordinal of the batch's first
    sample in the stream.  -> state = (best_d (K,C), best_src (K,C,2) int32, cand (K,C,L)): per shapelet the smallest distance
    so far, the (sample ordinal, window) that attains it -- the lowest on ties -- and a bit-exact copy of that window of xn.
    state None: allocated and overwritten (best_d = +inf, best_src = -1 where no sample has a window); given: updated where this
    batch is strictly nearer.  Bitwise repeatable; no gradient."""
    name = "shapelet_project_step"
    xn, d, t = _project_inputs(name, xn, d, t)
    B, C, T = xn.shape
    K, Cw, Lw = (int(v) for v in w_shape)
    if Cw != C:
        raise _lib.IgnError(f"{name}: the shapelets have {Cw} channels, the input has {C}")
    state, accumulate = _project_state(name, xn.device, (K, C, Lw), state)
    _lib.check(_lib.lib().ign_shapelet_project_step(_ptr(xn), _ptr(d), _ptr(t), d.shape[1], int(col0), int(sample0), _ptr(state[0]),
                                                    _ptr(state[1]), _ptr(state[2]), accumulate, B, C, T, K, Lw, int(stride), _stream()),
               "ign_shapelet_project_step")
    return state


def shapelet_project_bank(xn, d, t, w_shapes, strides, sample0, states=None):
    """shapelet_project_step for every length group of a bank, the groups' columns following each other from 0 in `d` / `t` as
    shapelet_bank lays them out: one ign_shapelet_project_step_bank call for up to BANK_MAX_GROUPS groups, group by group above.
    `states`: None or one state per group (all given or none).  -> list of states."""
    name = "shapelet_project_bank"
    G = len(w_shapes)
    col0s, col0 = [], 0
    for K, C, _ in w_shapes:
        col0s.append(col0)
        col0 += int(K) * int(C)
    if G > BANK_MAX_GROUPS or G == 0:
        states = states or [None] * G
        return [shapelet_project_step(xn, d, t, col0s[g], w_shapes[g], strides[g], sample0, states[g]) for g in range(G)]
    xn, d, t = _project_inputs(name, xn, d, t)
    B, C, T = xn.shape
    if any(int(s[1]) != C for s in w_shapes):
        raise _lib.IgnError(f"{name}: the shapelets have {[int(s[1]) for s in w_shapes]} channels, the input has {C}")
    if states is not None and (len(states) != G or any(s is None for s in states)):
        raise _lib.IgnError(f"{name}: pass one state per group (accumulate) or none at all (overwrite)")
    new = [_project_state(name, xn.device, w_shapes[g], states[g] if states is not None else None)[0] for g in range(G)]
    ints = ctypes.c_int * G
    _lib.check(_lib.lib().ign_shapelet_project_step_bank(
        _ptr(xn), _ptr(d), _ptr(t), d.shape[1], G, ints(*col0s), int(sample0), _pv([s[0] for s in new]), _pv([s[1] for s in new]),
        _pv([s[2] for s in new]), 0 if states is None else 1, B, C, T, ints(*[int(s[0]) for s in w_shapes]),
        ints(*[int(s[2]) for s in w_shapes]), ints(*[int(s) for s in strides]), _stream()), "ign_shapelet_project_step_bank")
    return new


def _evidence_target(name, target, B, N, bad=None):
    """The explained class per sample as the evidence kernels take it: int32 (B,) on the GPU, every entry inside [0, N).  `bad`: a
    further 0-dim device flag with the message to raise when it is set, read in the same device-to-host copy."""
    if not torch.is_tensor(target) or not target.is_cuda or target.dtype not in (torch.int32, torch.int64) \
            or tuple(target.shape) != (B,):
        what = f"{target.dtype} {tuple(target.shape)} on {target.device}" if torch.is_tensor(target) else type(target).__name__
        raise _lib.IgnError(f"{name}: target must be an integer tensor of shape ({B},) on the GPU, got {what}")
    flags = [((target < 0) | (target >= N)).any()] + ([bad[0]] if bad is not None else [])
    flags = torch.stack(flags).tolist()
    if flags[0]:
        raise _lib.IgnError(f"{name}: target outside [0, {N}): {target.tolist()}")
    if bad is not None and flags[1]:
        raise _lib.IgnError(f"{name}: {bad[1]()}")
    return target.to(torch.int32).contiguous()


_EVIDENCE_TW = {}          # (device, Ks, Ls, strides, C, T) -> int32 (ld,): windows per feature column, for the check of t


def _evidence_scale(name, scale, B):
    if scale is None:
        return None
    _need_gpu(name, scale)
    if tuple(scale.shape) != (B,):
        raise _lib.IgnError(f"{name}: scale must be a float32 tensor of shape ({B},), got {tuple(scale.shape)}")
    return scale.detach().contiguous()


def shapelet_evidence(p, t, W, target, Ks, Ls, strides, C, T, scale=None):
    """The linear-head shapelet expert's share of the logit of class target[b], laid out over the input (ign_shapelet_evidence_bank;
    the rule is csrc/ign_evidence.h, restated in utils/evidence.py:evidence_rule and equal to it bit for bit) -> (B,T,C) float32.
    `p` (B,ld) float32 and `t` (B,ld) int32: P and Tstar of shapelet_bank(..., return_tstar=True), feature order g*K*C + k*C + c;
    `W` (N,ld) the head's weight; `target` (B,) integer tensor on the GPU; `Ks`, `Ls`, `strides`: shapelets, length and window step
    of each length group; `scale`: None or a float32 (B,) factor per sample (the gate value), applied once after the sum.
    Feature f contributes fl(fl(W[n_b,f] * p[b,f]) * fl(1/L_g)) to every sample of its matched window [t*stride, t*stride + L) on its electrode;
    t = -1 (no window under --mask_padding) contributes nothing.  Nothing is launched when an argument is refused: a target outside
    [0, N), a `t` outside [-1, Tw_g), shapes that do not fit.  No gradient."""
    name = "shapelet_evidence"
    _need_gpu(name, p, W, scale)
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.int32:
        what = f"{t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise _lib.IgnError(f"{name}: t must be an int32 tensor on the GPU, got {what}")
    G = len(Ks)
    if not 1 <= G <= BANK_MAX_GROUPS or len(Ls) != G or len(strides) != G:
        raise _lib.IgnError(f"{name}: {G} groups (1..{BANK_MAX_GROUPS}) with {len(Ls)} lengths and {len(strides)} strides")
    Ks, Ls, strides, C, T = [int(k) for k in Ks], [int(v) for v in Ls], [int(s) for s in strides], int(C), int(T)
    if C < 1 or T < 1 or min(Ks) < 1 or min(strides) < 1 or min(Ls) < 1 or max(Ls) > T:
        raise _lib.IgnError(f"{name}: K={Ks} L={Ls} stride={strides} do not fit C={C}, T={T}")
    ld = sum(Ks) * C
    if p.dim() != 2 or p.shape[1] != ld or t.shape != p.shape or W.dim() != 2 or W.shape[1] != ld:
        raise _lib.IgnError(f"{name}: p, t must be (B,{ld}) and W (N,{ld}) for K={Ks}, C={C}; got {tuple(p.shape)}, {tuple(t.shape)}, "
                            f"{tuple(W.shape)}")
    B, N = p.shape[0], W.shape[0]
    out = torch.empty(B, T, C, device=p.device, dtype=torch.float32)
    if B == 0:
        return out
    p, t, W = p.detach().contiguous(), t.contiguous(), W.detach().contiguous()
    Tws = [(T - Ls[g]) // strides[g] + 1 for g in range(G)]
    col0s = [sum(Ks[:g]) * C for g in range(G)]
    key = (p.device, tuple(Ks), tuple(Ls), tuple(strides), C, T)
    tw = _EVIDENCE_TW.get(key)
    if tw is None:
        if len(_EVIDENCE_TW) >= 16:
            _EVIDENCE_TW.clear()
        tw = _EVIDENCE_TW[key] = torch.cat([torch.full((Ks[g] * C,), Tws[g], dtype=torch.int32) for g in range(G)]).to(p.device)
    # device data is checked here, with the target, in one device-to-host copy: the launch below trusts neither
    target = _evidence_target(name, target, B, N, bad=(((t < -1) | (t >= tw)).any(), lambda: (
        f"a match location outside [-1, Tw_g) with Tw = {Tws}: per group (min, max) = "
        f"{[(int(t[:, c0:c0 + k * C].min()), int(t[:, c0:c0 + k * C].max())) for c0, k in zip(col0s, Ks)]}")))
    scale = _evidence_scale(name, scale, B)
    ints, floats = ctypes.c_int * G, ctypes.c_float * G
    import numpy as np
    invL = [float(np.float32(1.0) / np.float32(v)) for v in Ls]
    _lib.check(_lib.lib().ign_shapelet_evidence_bank(_ptr(p), _ptr(t), _ptr(W), _ptr(target), _ptr(scale), ld, G, ints(*Ks), ints(*Ls),
                                                     ints(*strides), ints(*col0s), floats(*invL), _ptr(out), B, T, C, N, _stream()),
               "ign_shapelet_evidence_bank")
    return out


def fcn_cam(y_last, a, b, head_w, target, scale=None):
    """Class activation map of the FCN expert on its last block's time axis (ign_bn_relu_cam_fwd) -> (B,Tl) float32:
    cam[b,t] = scale[b] * (1/Tl) * sum_c head_w[target[b], c] * relu(a_c * y_last[b,t,c] + b_c), so cam.sum(1) + bias[target] is the
    expert's logit.  `y_last` (B,Tl,Cl) the raw output of the last convolution and `a`, `b` (Cl,) its eval-mode BatchNorm affine
    (what FullyConvNetwork.keep_last leaves in `last_block`), `head_w` (N,Cl), `target` (B,) integer tensor on the GPU, `scale` None
    or float32 (B,).  Cl % 4 == 0, Cl <= 1024.  No gradient."""
    name = "fcn_cam"
    _need_gpu(name, y_last, a, b, head_w, scale)
    if y_last.dim() != 3 or head_w.dim() != 2:
        raise _lib.IgnError(f"{name}: y_last must be (B,Tl,Cl) and head_w (N,Cl), got {tuple(y_last.shape)} and {tuple(head_w.shape)}")
    B, Tl, Cl = y_last.shape
    N = head_w.shape[0]
    if Cl % 4 or not 4 <= Cl <= 1024 or Tl < 1 or tuple(a.shape) != (Cl,) or tuple(b.shape) != (Cl,) or head_w.shape[1] != Cl:
        raise _lib.IgnError(f"{name}: y_last {tuple(y_last.shape)} needs Tl >= 1, Cl % 4 == 0, Cl <= 1024, a and b of shape ({Cl},) and "
                            f"head_w (N,{Cl}); got a {tuple(a.shape)}, b {tuple(b.shape)}, head_w {tuple(head_w.shape)}")
    cam = torch.empty(B, Tl, device=y_last.device, dtype=torch.float32)
    if B == 0:
        return cam
    target = _evidence_target(name, target, B, N)
    scale = _evidence_scale(name, scale, B)
    _lib.check(_lib.lib().ign_bn_relu_cam_fwd(_ptr(y_last.detach().contiguous()), _ptr(a.detach().contiguous()),
                                              _ptr(b.detach().contiguous()), _ptr(head_w.detach().contiguous()), _ptr(target),
                                              _ptr(scale), _ptr(cam), B, Tl, Cl, N, _stream()), "ign_bn_relu_cam_fwd")
    return cam


def cam_spread(cam, R):
    """cam (B,Tl) on the FCN's last time axis -> (B,T) on the input axis, T = Tl + R - 1 (ign_cam_spread): every cam[b,t] spread
    evenly over the R = k1 + k2 + k3 - 2 input samples it saw, out[b,s] = fl(fl(1/R) * sum_{t = max(0,s-R+1)}^{min(s,Tl-1)} cam[b,t])
    with t ascending -- bitwise equal to utils/evidence.py:cam_spread_rule; out.sum(1) is cam.sum(1) up to rounding."""
    name = "cam_spread"
    _need_gpu(name, cam)
    R = int(R)
    if cam.dim() != 2 or cam.shape[1] < 1 or R < 1:
        raise _lib.IgnError(f"{name}: cam must be (B,Tl) with Tl >= 1 and R >= 1, got {tuple(cam.shape)} and R={R}")
    B, Tl = cam.shape
    out = torch.empty(B, Tl + R - 1, device=cam.device, dtype=torch.float32)
    if B == 0:
        return out
    import numpy as np
    _lib.check(_lib.lib().ign_cam_spread(_ptr(cam.detach().contiguous()), _ptr(out), B, Tl, R, float(np.float32(1.0) / np.float32(R)),
                                         _stream()), "ign_cam_spread")
    return out


RANK_MAX_K = 32               # IGN_RANK_MAX_K (include/ign_abi.h): most thresholds one ign_rank_threshold call finds per sample


def _need_plain(name, what, t, dtype, dim):
    """An input of the faithfulness ops: a contiguous tensor of `dtype` with `dim` axes on the GPU that needs no gradient."""
    if not torch.is_tensor(t) or not t.is_cuda:
        where = f"on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise _lib.IgnError(f"{name}: {what} must be a tensor on the GPU, got {where} (there is no CPU path: the numpy restatement "
                            f"lives in utils/faithfulness.py)")
    if t.dtype != dtype:
        raise _lib.IgnError(f"{name}: {what} must be {dtype}, got {t.dtype}")
    if t.dim() != dim or not t.is_contiguous():
        raise _lib.IgnError(f"{name}: {what} must be a contiguous tensor with {dim} axes, got shape {tuple(t.shape)} strides "
                            f"{t.stride()}")
    if t.requires_grad:
        raise _lib.IgnError(f"{name}: {what} requires a gradient; ranking and perturbing act on data (there is no backward pass)")


def rank_threshold(score, k, lengths=None):
    """Per sample the thresholds of its top-k sets under a score map (ign_rank_threshold; the rule is utils/faithfulness.py:rank_rule,
    equal to it bit for bit) -> (thr_key, thr_idx), both int32 (B,nk); thr_key holds the bits of the uint32 key.
    `score`: float32 (B,T,Cs) -- a score per cell (Cs = C) or per time step (Cs = 1), flat index i = t*Cs + c; `k`: int32 (B,nk),
    nk <= RANK_MAX_K, clamped to [0, n_b] on the device; `lengths`: int32 (B,) or None -- sample b has n_b = clamp(len_b, 0, T) * Cs
    scores.  Elements are ordered by descending key (the order-preserving uint32 of the float's bits: -0 below +0, NaNs at the
    ends), ties to the lowest flat index; the k-th element's (key, index) is returned, (0xffffffff, -1) for k = 0.  Everything is
    device data: no host sync, one launch for all nk thresholds."""
    name = "rank_threshold"
    _need_plain(name, "score", score, torch.float32, 3)
    _need_plain(name, "k", k, torch.int32, 2)
    B, T, Cs = score.shape
    nk = k.shape[1]
    if k.shape[0] != B or not 1 <= nk <= RANK_MAX_K:
        raise _lib.IgnError(f"{name}: k must be ({B}, nk) with nk in 1..{RANK_MAX_K}, got {tuple(k.shape)}")
    thr_key = torch.empty(B, nk, device=score.device, dtype=torch.int32)
    thr_idx = torch.empty(B, nk, device=score.device, dtype=torch.int32)
    if B == 0:
        return thr_key, thr_idx
    if lengths is not None:
        lengths = _lengths(name, lengths, B)
    _lib.check(_lib.lib().ign_rank_threshold(_ptr(score), _ptr(k), _ptr(lengths), _ptr(thr_key), _ptr(thr_idx), B, T, Cs, nk,
                                             _stream()), "ign_rank_threshold")
    return thr_key, thr_idx


def _fill_bc(name, fill, B, C):
    """The replacement values of `perturb` and `occlude`: None (0.0) or a plain float32 (B,C) tensor."""
    if fill is not None:
        _need_plain(name, "fill", fill, torch.float32, 2)
        if tuple(fill.shape) != (B, C):
            raise _lib.IgnError(f"{name}: fill must be ({B},{C}), got {tuple(fill.shape)}")


def perturb(x, score, thr_key, thr_idx, j, fill=None, insert=False, lengths=None):
    """The batch with each sample's top-k cells replaced (ign_perturb_btc; the rule is utils/faithfulness.py:perturb_rule, equal to it
    bit for bit) -> a new (B,T,C) tensor.  `x`: float32 (B,T,C); `score`: the map the thresholds were taken from, (B,T,C) or (B,T,1);
    `thr_key`, `thr_idx`: int32 (B,nk) of rank_threshold; `j`: a host integer in [0, nk), the column used; `fill`: float32 (B,C) or
    None for 0.0; `insert`: keep the selected cells and replace the others; `lengths`: int32 (B,) or None -- from lengths[b] on the
    sample is copied through.  A cell is selected iff key > thr_key, or key == thr_key and its flat index <= thr_idx.  Every argument
    but `j` and `insert` is device data, so the call may be captured."""
    name = "perturb"
    _need_plain(name, "x", x, torch.float32, 3)
    _need_plain(name, "score", score, torch.float32, 3)
    _need_plain(name, "thr_key", thr_key, torch.int32, 2)
    _need_plain(name, "thr_idx", thr_idx, torch.int32, 2)
    B, T, C = x.shape
    Cs = score.shape[2]
    if tuple(score.shape[:2]) != (B, T) or Cs not in (1, C):
        raise _lib.IgnError(f"{name}: score must be ({B},{T},{C}) or ({B},{T},1) for x {tuple(x.shape)}, got {tuple(score.shape)}")
    nk = thr_key.shape[1]
    if thr_key.shape[0] != B or thr_idx.shape != thr_key.shape or not 1 <= nk <= RANK_MAX_K:
        raise _lib.IgnError(f"{name}: thr_key and thr_idx must be ({B}, nk) with nk in 1..{RANK_MAX_K}, got {tuple(thr_key.shape)} "
                            f"and {tuple(thr_idx.shape)}")
    j = int(j)
    if not 0 <= j < nk:
        raise _lib.IgnError(f"{name}: j = {j} outside [0, {nk})")
    _fill_bc(name, fill, B, C)
    out = torch.empty_like(x)
    if B == 0:
        return out
    if lengths is not None:
        lengths = _lengths(name, lengths, B)
    _lib.check(_lib.lib().ign_perturb_btc(_ptr(x), _ptr(score), _ptr(thr_key), _ptr(thr_idx), j, nk, _ptr(fill), _ptr(lengths),
                                          _ptr(out), int(bool(insert)), B, T, C, Cs, _stream()), "ign_perturb_btc")
    return out


OCC_MAX_COVER = 64            # IGN_OCC_MAX_COVER (include/ign_abi.h): most windows over one time step that ign_occlusion_spread adds


_OCC_CONST = {}               # (kind, bytes, device) -> the device copy of a small host table; kept, so a captured launch's pointer stays good


def _occ_const(kind, host, device):
    key = (kind, host.tobytes(), str(device))
    if key not in _OCC_CONST:
        _OCC_CONST[key] = torch.from_numpy(host).to(device)
    return _OCC_CONST[key]


def _occ_gid(name, gid, groups, C, device):
    """The electrode groups as the kernels take them, an int32 (C,) tensor on `device`, made from -- and checked on -- HOST data (a
    sequence, a numpy array or a CPU tensor): the kernels never index with a value outside [0, groups).  The device copy of a table
    is made once, so a second call copies nothing and may be captured."""
    import numpy as np
    groups = int(groups)
    if torch.is_tensor(gid) and gid.is_cuda:
        raise _lib.IgnError(f"{name}: gid must be host data (it is checked on the host before any launch), got a tensor on {gid.device}")
    host = np.asarray(gid)
    if host.shape != (C,) or host.dtype.kind not in "iu":
        raise _lib.IgnError(f"{name}: gid must be {C} integers, one group per electrode, got {host.dtype} {host.shape}")
    if groups < 1 or (host < 0).any() or (host >= groups).any():
        raise _lib.IgnError(f"{name}: gid must lie in [0, groups) with groups = {groups} >= 1, got {int(host.min())} .. {int(host.max())}")
    return _occ_const("gid", np.ascontiguousarray(host, dtype=np.int32), device), groups


def occlude(x, p0, count, gid, groups, window, stride, fill=None, lengths=None):
    """`count` occluded copies of every sample (ign_occlude_btc; the rule is utils/occlusion.py:occlude_rule, equal to it bit for bit)
    -> a new (B*count, T, C) tensor, row b*count + q the copy of sample b under patch p0 + q.  `x`: float32 (B,T,C); `gid`: C integers
    in [0, groups), a host array (or a tensor, copied to the host and checked there); `window`, `stride`: the time grid of
    utils.occlusion.grid (0: the whole series / the window); patch p = i*groups + g hides steps [i*S, min(i*S + W, len_b)) of the
    electrodes in group g behind `fill` (float32 (B,C), None: 0.0); `lengths`: int32 (B,) or None.  One read of x, `count` writes;
    every scalar is a host integer, so the call may be captured."""
    from utils.occlusion import grid
    name = "occlude"
    _need_plain(name, "x", x, torch.float32, 3)
    B, T, C = x.shape
    W, S, nt = grid(T, window, stride)
    gid_d, G = _occ_gid(name, gid, groups, C, x.device)
    p0, count = int(p0), int(count)
    if p0 < 0 or count < 1 or p0 + count > nt * G:
        raise _lib.IgnError(f"{name}: patches {p0} .. {p0 + count - 1} outside [0, {nt * G}) ({nt} windows x {G} groups)")
    _fill_bc(name, fill, B, C)
    out = torch.empty(B * count, T, C, device=x.device, dtype=torch.float32)
    if B == 0:
        return out
    if lengths is not None:
        lengths = _lengths(name, lengths, B)
    _lib.check(_lib.lib().ign_occlude_btc(_ptr(x), _ptr(fill), _ptr(lengths), _ptr(gid_d), _ptr(out), p0, count, G, W, S, nt, B, T, C,
                                          _stream()), "ign_occlude_btc")
    return out


def occlusion_spread(drop, gid, groups, window, stride, T, lengths=None):
    """The drops of the class score laid back over the cells that were hidden (ign_occlusion_spread; the rule is
    utils/occlusion.py:spread_rule, equal to it bit for bit) -> a new (B,T,C) tensor.  `drop`: float32 (B, nt*groups), column
    i*groups + g the drop under window i on group g; `gid`, `groups`, `window`, `stride`, `lengths` as in `occlude`.  A cell inside
    the sample's length takes the mean of the drops of the windows over its step on its electrode's group (added in ascending window
    order, times the host's float32 1 / count); beyond the length the map is +0.0."""
    from utils.occlusion import grid, inv_table
    name = "occlusion_spread"
    _need_plain(name, "drop", drop, torch.float32, 2)
    T = int(T)
    if T < 1:
        raise _lib.IgnError(f"{name}: T = {T}, need at least one time step")
    W, S, nt = grid(T, window, stride)
    cover = -(-W // S)
    if cover > OCC_MAX_COVER:
        raise _lib.IgnError(f"{name}: window {W} / stride {S} put {cover} windows over a step, more than {OCC_MAX_COVER} "
                            f"(IGN_OCC_MAX_COVER)")
    C = len(gid) if hasattr(gid, "__len__") else -1
    gid_d, G = _occ_gid(name, gid, groups, C, drop.device)
    B = drop.shape[0]
    if drop.shape[1] != nt * G:
        raise _lib.IgnError(f"{name}: drop must be ({B}, {nt * G}) for {nt} windows x {G} groups, got {tuple(drop.shape)}")
    out = torch.empty(B, T, C, device=drop.device, dtype=torch.float32)
    if B == 0:
        return out
    if lengths is not None:
        lengths = _lengths(name, lengths, B)
    inv_d = _occ_const("inv", inv_table(cover), drop.device)
    _lib.check(_lib.lib().ign_occlusion_spread(_ptr(drop), _ptr(gid_d), _ptr(lengths), _ptr(inv_d), _ptr(out), G, W, S, nt, B, T, C,
                                               _stream()), "ign_occlusion_spread")
    return out


class SbmFn(torch.autograd.Function):
    """The shapelet bottleneck model behind the instance norm as ONE autograd node: shapelet bank (every length group) ->
    linear class head (optional) -> both regularisers (IGN/model/Shapelet.py:190-210, 217-230).

    forward(xn, cfg, W, w_0..w_{G-1}[, thr_0..thr_{G-1}]) -> (P, Dmin, Tstar | None, reg, out | None)
      cfg = (eps, mode, strides, G, lambda_reg, lambda_div, fuse_head, want_tstar, reg_workspace)
      reg (1,) = lambda_reg * mean|W| + lambda_div * sum_g diversity_g -- value AND gradients from one launch
      (ign_sbm_reg_fwd_bwd); out = P W^T when fuse_head.
    Why one node: W and every w_g receive a gradient from the data path and one from a regulariser.  As separate nodes
    autograd adds the two with one accumulate kernel per parameter and the regularisers cost ~30 small launches per step
    (abs / mean / mul, four diversity launches, their sums and products, backward mirrors).  Here the head's weight-gradient
    kernel and the bank's reduction launch add `upstream * regulariser gradient` in their epilogues: the backward is
    head_bwd (2 launches) + G shapelet launches + 1 reduction, with no torch kernel in between."""

    @staticmethod
    def forward(ctx, xn, cfg, W, *params):
        eps, mode, strides, G, lam_reg, lam_div, fuse_head, want_tstar, reg_ws = cfg
        xn, bank, P, D = _node_forward(xn, (W,), params, G, eps, mode, strides, ctx.needs_input_grad[0],
                                       any(ctx.needs_input_grad[2:]), gpu_name="sbm", grad_name="sbm")
        W = W.contiguous()
        ws = [s.w for s in bank.groups]
        L = _lib.lib()
        Tstar = bank.cat_tstar() if want_tstar else None
        # regularisers: value + gradients, one launch
        use_div = lam_div > 0.0
        gWreg = torch.empty_like(W)
        gdiv = [torch.empty_like(w) for w in ws] if use_div else None
        reg = torch.empty(1, device=xn.device, dtype=torch.float32)
        Gd = G if use_div else 0
        _lib.check(L.ign_sbm_reg_fwd_bwd(_ptr(W), _ptr(gWreg), W.numel(), float(lam_reg), Gd, bank.ws, _pv(gdiv) if use_div else None,
                                         bank.Ks, bank.Ls, bank.C, float(lam_div), 1e-6, _ptr(reg), _ptr(reg_ws), _stream()),
                   "ign_sbm_reg_fwd_bwd")
        out = None
        if fuse_head:
            N, F_ = W.shape
            _check_classes("sbm head", N)
            out = torch.empty(bank.B, N, device=xn.device, dtype=torch.float32)
            _lib.check(L.ign_head_fwd(_ptr(P), _ptr(W), None, _ptr(out), bank.B, F_, N, P.stride(0), _stream()), "ign_head_fwd")
        ctx.set_materialize_grads(False)
        nd = [D] + ([Tstar] if Tstar is not None else [])
        ctx.mark_non_differentiable(*nd)
        ctx.bank, ctx.fuse_head, ctx.gdiv = bank, fuse_head, gdiv
        ctx.save_for_backward(xn, P, D, W, gWreg, *ws)
        return P, D, Tstar, reg, out

    @staticmethod
    def backward(ctx, gP, gD, gT, greg, gout):
        bank, fuse_head, gdiv = ctx.bank, ctx.fuse_head, ctx.gdiv
        if not bank.need_grad:
            raise _lib.IgnError("shapelet backward called but the forward ran without saving distances")
        xn, P, D, W, gWreg = ctx.saved_tensors[:5]
        L = _lib.lib()
        greg = greg.contiguous().reshape(1) if greg is not None else None
        need_x, need_W, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[2], any(ctx.needs_input_grad[3:])
        gW = None
        if fuse_head and gout is not None:
            N, F_ = W.shape
            gout = gout.contiguous()
            gPh = torch.empty_like(P)
            gW = torch.empty_like(W) if (need_W or not need_x) else None       # (frozen head under an input gradient: gX only)
            _lib.check(L.ign_head_bwd_acc(_ptr(gout), _ptr(P), _ptr(W), _ptr(gPh), _ptr(gW), None,
                                          _ptr(gWreg) if (greg is not None and gW is not None) else None, _ptr(greg), bank.B, F_, N,
                                          P.stride(0), _stream()),
                       "ign_head_bwd_acc")
            gP = gPh if gP is None else gPh + gP
        elif greg is not None and need_W:
            gW = gWreg * greg
        add = gdiv if (gdiv is not None and greg is not None) else None
        gxn, grads_w, grads_t = _node_backward(bank, xn, gP, P, D, need_x, need_p, add, greg if add is not None else None)
        if gP is None and add is not None:             # nothing reached the gate outputs: only the regulariser moves the shapelets
            grads_w = [gd * greg for gd in add]
        return (gxn, None, gW, *grads_w, *grads_t)


def _bl_strides(t, name):
    """(B,L,H,E) tensor -> element strides of the batch and sequence axes; inner (H,E) block must be dense."""
    B, L, H, E = t.shape
    if t.stride(3) != 1 or t.stride(2) != E:
        raise _lib.IgnError(f"attention: {name} needs unit stride over E and stride E over H, got {t.stride()}")
    return t.stride(0), t.stride(1)


def _attn_operand_ok(t):
    """What the attention entry points take as q / k / v (attn_check): a dense (H, E) block, batch and sequence strides that are
    positive multiples of 4 elements, a 16-byte aligned base."""
    return (t.stride(3) == 1 and t.stride(2) == t.shape[3] and t.stride(0) > 0 and t.stride(0) % 4 == 0
            and t.stride(1) > 0 and t.stride(1) % 4 == 0 and t.data_ptr() % 16 == 0)


def _attn_operand(t):
    """t itself where the kernels can read it in place (a strided view of a packed projection), else a copy.  A batch-expanded
    operand (stride 0) is copied; so is one that torch already calls contiguous but the kernels refuse (a misaligned base, a
    size-1 axis with stride 0), which `.contiguous()` would hand back unchanged."""
    if _attn_operand_ok(t):
        return t
    c = t.contiguous()
    return c if _attn_operand_ok(c) else t.clone(memory_format=torch.contiguous_format)


# Attention dropout (include/ign_abi.h, "Attention dropout"): arithmetic selectors of ign_attn_fwd_dropout / ign_attn_bwd_dropout
ATTN_MATH_F32, ATTN_MATH_X6, ATTN_MATH_BF16, ATTN_MATH_H3 = 0, 1, 2, 3


def dropout_threshold(p):
    """-> (thr, s) of the kernels' keep rule for a dropout rate p (as the fp32 the C ABI receives): keep <=> a 16-bit Philox
    halfword >= thr, thr = round(p * 65536); kept probabilities are scaled by s = 65536 / (65536 - thr) (fp32)."""
    p32 = ctypes.c_float(p).value
    if not (0.0 <= p32 < 1.0):
        raise ValueError(f"attention dropout p = {p} outside [0, 1)")
    thr = round(p32 * 65536.0)                  # exact product; round half to even like rintf
    if thr >= 65536:
        raise ValueError(f"attention dropout p = {p} rounds to a keep rate of 0")
    return thr, ctypes.c_float(ctypes.c_float(65536.0).value / float(65536 - thr)).value


def _dropout_seed(p):
    """A fresh 64-bit seed from torch's default generator (torch.manual_seed makes a step reproducible to the bit).  A seed passed
    by value would be baked into a captured hipGraph and every replay would reuse one mask: refused while capturing."""
    dropout_threshold(p)
    if torch.cuda.is_current_stream_capturing():
        raise _lib.IgnError("attention dropout p > 0 inside a hipGraph capture: the per-call seed would be frozen into the graph "
                            "(run the step eagerly, or with attention dropout 0)")
    lo, hi = torch.randint(0, 2 ** 32, (2,), dtype=torch.int64).tolist()
    return lo | (hi << 32)


def _attn_arith(E, autocast, bwd, grad=False):
    """The arithmetic (ATTN_MATH_*) of the attention forward (bwd False) or backward at head width E: the one place that reads
    ATTN_MATH; the split kernels follow the dense layers (_dense_arith) onto the fp16 planes.
    grad: the forward of a call that will be differentiated.  Where the backward runs the fp32-MFMA kernels (E = 128) that forward
    runs them too: the backward forms p = exp(s - lse) from ITS scores, and dq = scale sum_j p_j (dP_j - delta) k_j cancels over the
    keys only as far as lse and delta = dO . out come from the same p.  An lse from the split forward differs per key by the fp32
    rounding of the score (2e-6 at |s| = 20), which rows of nearly collinear keys amplify (9e-5 of max |dq| against 1e-5 with one
    family: tests/test_gpu_attn_edges.py, the rising / falling regimes).  Up to E = 64 forward and backward share a family.
    The caller passes ctx.needs_input_grad, which ignores the grad mode: a leaf that requires grad takes this forward under
    torch.no_grad() too (slower, never wrong).  Cost at E = 128: DESIGN 4.4."""
    if grad and not bwd and _attn_arith(E, autocast, True) == ATTN_MATH_F32:
        return ATTN_MATH_F32
    if autocast and E <= 64:
        return ATTN_MATH_BF16     # inside an autocast region (the reference's default mode): operands rounded to bf16, one product
    if ATTN_MATH == "bf16x6" and _dense_arith(False) == GEMM_H3 and E <= 64:
        return ATTN_MATH_H3       # two fp16 planes of power-of-two-scaled operands, three products; needs the magnitude bounds
    if ATTN_MATH == "bf16x6" and (E <= 64 or not bwd):
        # split-bf16 products on the bf16 matrix cores (fp32 accuracy); the backward up to E = 64 only (E = 128 exceeds its
        # register budget: the fp32-MFMA backward is faster there)
        return ATTN_MATH_X6
    return ATTN_MATH_F32          # "f32": the fp32-MFMA kernels


_ATTN_FWD = {ATTN_MATH_F32: "ign_attn_fwd", ATTN_MATH_X6: "ign_attn_fwd_x6", ATTN_MATH_BF16: "ign_attn_fwd_bf16"}
_ATTN_BWD = {ATTN_MATH_F32: "ign_attn_bwd", ATTN_MATH_X6: "ign_attn_bwd_x6", ATTN_MATH_BF16: "ign_attn_bwd_bf16"}


def _attn_fwd(ctx, q, k, v, out, lse):
    """The forward launch of AttentionFn / PackedAttentionFn, from what their forward stored on ctx: arith, p, seed, scale, the
    six batch / sequence strides and the three H3 bounds (None otherwise).  p = 0 keeps to the dropout-free entry points."""
    B, L, H, E = q.shape
    bq, bk, bv = (_ptr(b) for b in ctx.bounds)
    if ctx.p > 0:
        name, tail = "ign_attn_fwd_dropout", (ctx.arith, bq, bk, bv, ctx.p, ctx.seed)
    elif ctx.arith == ATTN_MATH_H3:
        name, tail = "ign_attn_fwd_h3", (bq, bk, bv)
    else:
        name, tail = _ATTN_FWD[ctx.arith], ()
    _lib.check(getattr(_lib.lib(), name)(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), B, L, k.shape[1], H, E, *ctx.strides,
                                         ctx.scale, _stream(), *tail), name)


def _attn_bwd(ctx, q, k, v, out, lse, gout, gq, gk, gv, g_strides):
    """The backward launch matching _attn_fwd; g_strides (0, 0): contiguous gradients, else the batch / sequence strides of a
    packed gradient buffer.  -> the H3 gradients' bound (max |gq|, |gk|, |gv| as the kernels store them), else None."""
    B, L, H, E = q.shape
    arith = ctx.bwd_arith
    delta = torch.empty(B, H, L, device=q.device, dtype=torch.float32)
    gmax = bgo = None
    if arith == ATTN_MATH_H3:
        gmax = _new_slot(q.device)
        bgo = tensor_bound(gout)
    bounds = (*(_ptr(b) for b in ctx.bounds), _ptr(bgo), _ptr(gmax))
    if ctx.p > 0:
        name, tail = "ign_attn_bwd_dropout", (arith, *g_strides, *bounds, ctx.p, ctx.seed)
    elif arith == ATTN_MATH_H3:
        name, tail = "ign_attn_bwd_h3", (*g_strides, *bounds)
    elif g_strides != (0, 0):
        name, tail = "ign_attn_bwd_x6_strided", (*g_strides, 1 if arith == ATTN_MATH_BF16 else 0)
    else:
        name, tail = _ATTN_BWD[arith], ()
    _lib.check(getattr(_lib.lib(), name)(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), _ptr(gout), _ptr(gq), _ptr(gk), _ptr(gv),
                                         _ptr(delta), B, L, k.shape[1], H, E, *ctx.strides, ctx.scale, _stream(), *tail), name)
    return gmax


class AttentionFn(torch.autograd.Function):
    """softmax(scale * Q K^T) V with q (B,L,H,E), k/v (B,S,H,E) -> (B,L,H,E); IGN/layers/SelfAttention_Family.py:56-75.
    dropout_p > 0: dropout on the attention probabilities inside the kernels, mask regenerated in the backward from `seed`.
    need_weights: also the (B,H,L,S) map dropout(softmax(scale * Q K^T)) of this call (ign_attn_probs), not differentiable."""

    @staticmethod
    def forward(ctx, q, k, v, scale, dropout_p=0.0, seed=0, need_weights=False):
        _need_gpu("attention", q, k, v)
        B, L, H, E = q.shape
        S = k.shape[1]
        q, k, v = _attn_operand(q), _attn_operand(k), _attn_operand(v)
        out = torch.empty(B, L, H, E, device=q.device, dtype=torch.float32)
        lse = torch.empty(B, H, L, device=q.device, dtype=torch.float32)
        ctx.strides = (*_bl_strides(q, "q"), *_bl_strides(k, "k"), *_bl_strides(v, "v"))
        autocast = torch.is_autocast_enabled()
        ctx.arith = _attn_arith(E, autocast, False, any(ctx.needs_input_grad[:3]))
        ctx.bwd_arith = _attn_arith(E, autocast, True)
        ctx.p, ctx.seed, ctx.scale = float(dropout_p), int(seed), float(scale)
        ctx.bounds = (tensor_bound(q), tensor_bound(k), tensor_bound(v)) if ctx.arith == ATTN_MATH_H3 else (None,) * 3
        _attn_fwd(ctx, q, k, v, out, lse)
        ctx.save_for_backward(q, k, v, out, lse)
        if not need_weights:
            return out
        # the map of this call: same q / k (after _attn_operand), lse, arithmetic, bounds and seed as the forward above
        attn = torch.empty(B, H, L, S, device=q.device, dtype=torch.float32)
        _lib.check(_lib.lib().ign_attn_probs(_ptr(q), _ptr(k), _ptr(lse), _ptr(attn), B, L, S, H, E, *ctx.strides[:4], ctx.scale,
                                             _stream(), ctx.arith, _ptr(ctx.bounds[0]), _ptr(ctx.bounds[1]), ctx.p, ctx.seed),
                   "ign_attn_probs")
        ctx.mark_non_differentiable(attn)
        ctx.set_materialize_grads(False)              # (else autograd would hand the backward a zero tensor of the map's size)
        return out, attn

    @staticmethod
    def backward(ctx, gout, gattn=None):
        if gout is None:                              # need_weights: only `out` carries a gradient
            return (None,) * 7
        q, k, v, out, lse = ctx.saved_tensors
        gout = gout.contiguous()
        gq = torch.empty(q.shape, device=q.device, dtype=torch.float32)
        gk = torch.empty(k.shape, device=q.device, dtype=torch.float32)
        gv = torch.empty_like(gk)
        gmax = _attn_bwd(ctx, q, k, v, out, lse, gout, gq, gk, gv, (0, 0))
        if gmax is not None:                          # one bound for the three
            gq, gk, gv = set_bound(gq, gmax), set_bound(gk, gmax), set_bound(gv, gmax)
        return gq, gk, gv, None, None, None, None


def _attn_out_bound(out, src, dropout_p):
    """f16x3: attach to `out` the bound of v taken from `src` (v, or the packed qkv whose bound bounds v; cached: no extra pass):
    a row of the output is a convex combination of rows of v, times the dropout scale s when p > 0."""
    if _attn_arith(out.shape[-1], torch.is_autocast_enabled(), False) == ATTN_MATH_H3:
        b = tensor_bound(src)
        set_bound(out, b if dropout_p == 0 else b * dropout_threshold(dropout_p)[1])


def attention(q, k, v, scale, dropout_p=0.0, need_weights=False):
    """dropout_p: attention dropout (callers pass p > 0 in training only); 0 takes the dropout-free kernels and draws nothing.
    need_weights=True returns (out, attn): attn (B, H, L, S) = dropout(softmax(scale * Q K^T)) of this very call (same operands,
    arithmetic, lse and dropout seed as `out`; one seed per call).  attn is NOT differentiable: it does not require grad, and the
    gradients of q, k, v are those of `out` alone.  need_weights=False launches, allocates and draws nothing more."""
    seed = 0 if dropout_p == 0 else _dropout_seed(dropout_p)
    res = AttentionFn.apply(q, k, v, scale, float(dropout_p), seed, need_weights)
    _attn_out_bound(res[0] if need_weights else res, v, dropout_p)
    return res


class PackedAttentionFn(torch.autograd.Function):
    """Self-attention on a packed projection qkv (B, L, 3, H, E) -> (B, L, H, E): q / k / v are read as strided views and the
    three gradients are written straight into one packed buffer (ign_attn_bwd_x6_strided), so a fused q/k/v Linear layer gets
    its output gradient without a stack / gather pass."""

    @staticmethod
    def forward(ctx, qkv, scale, dropout_p=0.0, seed=0):
        _need_gpu("attention", qkv)
        qkv = qkv.contiguous()
        B, L, three, H, E = qkv.shape
        out = torch.empty(B, L, H, E, device=qkv.device, dtype=torch.float32)
        lse = torch.empty(B, H, L, device=qkv.device, dtype=torch.float32)
        ctx.strides = (qkv.stride(0), qkv.stride(1)) * 3
        autocast = torch.is_autocast_enabled()
        ctx.arith, ctx.bwd_arith = _attn_arith(E, autocast, False), _attn_arith(E, autocast, True)
        ctx.p, ctx.seed, ctx.scale = float(dropout_p), int(seed), float(scale)
        bound = tensor_bound(qkv) if ctx.arith == ATTN_MATH_H3 else None   # one pass: it bounds q, k and v alike
        ctx.bounds = (bound,) * 3
        _attn_fwd(ctx, qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], out, lse)
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    def backward(ctx, gout):
        qkv, out, lse = ctx.saved_tensors
        gout = gout.contiguous()
        gqkv = torch.empty_like(qkv)
        gmax = _attn_bwd(ctx, qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], out, lse, gout, gqkv[:, :, 0], gqkv[:, :, 1], gqkv[:, :, 2],
                         ctx.strides[:2])
        # the projection's backward GEMMs scale their dL/dy operand by the H3 bound without a pass over it
        return (gqkv if gmax is None else set_bound(gqkv, gmax)), None, None, None


def attention_packed(qkv, scale, dropout_p=0.0):
    """softmax(scale q k^T) v for qkv (B, L, 3, H, E); dropout_p as in `attention`.  The packed kernels are the split ones: where
    the configuration runs the fp32-MFMA backward outside autocast (ATTN_MATH "f32", or E > 64), the unpacked path."""
    if _attn_arith(qkv.shape[-1], False, True) == ATTN_MATH_F32:
        return attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], scale, dropout_p)
    seed = 0 if dropout_p == 0 else _dropout_seed(dropout_p)
    out = PackedAttentionFn.apply(qkv, scale, float(dropout_p), seed)
    _attn_out_bound(out, qkv, dropout_p)
    return out


class HeadLinearFn(torch.autograd.Function):
    """Skinny expert-head GEMM x (B,F) @ W(N,F)^T + bias -> (B,N) on ign_head_fwd/bwd."""

    @staticmethod
    def forward(ctx, x, w, bias):
        _need_gpu("head_linear", x, w, bias)
        x = x if (x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0) else x.contiguous()
        w = w.contiguous()
        B, F_ = x.shape
        N = w.shape[0]
        out = torch.empty(B, N, device=x.device, dtype=torch.float32)
        _lib.check(_lib.lib().ign_head_fwd(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), B, F_, N, x.stride(0), _stream()),
                   "ign_head_fwd")
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        B, F_ = x.shape
        N = w.shape[0]
        g = g.contiguous()
        gx = torch.empty(B, F_, device=x.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        gb = torch.empty(N, device=x.device, dtype=torch.float32) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        if gb is not None and gw is None:
            gw = torch.empty_like(w)
        _lib.check(_lib.lib().ign_head_bwd(_ptr(g), _ptr(x), _ptr(w), _ptr(gx), _ptr(gw), _ptr(gb), B, F_, N, x.stride(0),
                                           _stream()), "ign_head_bwd")
        # gx was written with row pitch x.stride(0); it is dense only if x was (the common case)
        if gx is not None and x.stride(0) != F_:
            raise _lib.IgnError("head_linear backward: padded input rows are not supported")
        return gx, (gw if ctx.needs_input_grad[1] else None), gb


def head_linear(x, w, bias=None):
    """nn.Linear with few outputs (class logits).  Shapes the streaming kernel does not cover go to torch's GEMM
    (still on the GPU; CPU tensors are refused)."""
    if not x.is_cuda:
        raise _lib.IgnError(f"head_linear: tensor on {x.device}; the product path runs on the MI355X only (no CPU fallback)")
    if x.dim() != 2 or x.shape[1] % 4 or not head_fits(x.shape[0], w.shape[0]) or x.dtype != torch.float32 \
            or w.dtype != torch.float32 or torch.is_autocast_enabled():
        return torch.nn.functional.linear(x, w, bias)
    return HeadLinearFn.apply(x, w, bias)


# Arithmetic of the dense-layer / convolution GEMMs outside an autocast region (include/ign_abi.h, "h3"):
#   "f16x3"  (default) operands scaled by a power of two from a device-side magnitude bound, split into two fp16 planes, three
#            products -- fp32-level accuracy against float64 like "bf16x6", at 1.5-1.6x its speed;
#   "bf16x6" three bf16 planes, six products.
GEMM_MATH = os.environ.get("IGN_GEMM_MATH", "f16x3")

_SLOT_POOL = {}


def _new_slot(device):
    """One zero-initialised float on `device`, cut from a pooled zero buffer (one fill launch per 256 slots).  While a hipGraph is
    being captured the slot gets its own fill INSIDE the graph: the kernels max into it atomically, so a slot zeroed once at
    allocation would carry the maximum over all earlier replays into every later one."""
    if torch.cuda.is_current_stream_capturing():
        return torch.zeros(1, device=device, dtype=torch.float32)
    pool = _SLOT_POOL.get(device)
    if pool is None or pool[1] >= pool[0].numel():
        pool = _SLOT_POOL[device] = [torch.zeros(256, device=device, dtype=torch.float32), 0]
    i = pool[1]
    pool[1] = i + 1
    return pool[0][i:i + 1]


def cached_bound(t):
    """The bound attached to `t` (one-element device tensor) if it still describes the tensor's contents, else None.  A bound
    that was MEASURED from the data in an earlier call (ign_absmax, ign_instnorm_fwd_amax) is not trusted while a hipGraph is
    being captured: the capture would bake in 'already known' and replay the example batch's bound for every later batch
    (GraphedTrainStep refills the same input tensors).  Bounds attached by a producer inside the captured region carry the
    flag `in_graph` and stay valid -- their kernels are part of the graph."""
    cb = getattr(t, "_ign_bound", None)
    if cb is None or cb[1] != t._version or cb[2] != t.data_ptr():
        return None
    if torch.cuda.is_current_stream_capturing() and not (len(cb) > 3 and cb[3]):
        return None
    return cb[0]


def tensor_bound(t):
    """A one-element device tensor holding an upper bound of max |t| -- what the fp16 GEMMs scale their operands by.  A producer
    that knows a bound attaches it (`set_bound`: LayerNorm's hard bound from its parameters); otherwise ONE pass over the tensor
    takes the exact maximum (ign_absmax), cached on the tensor object for as long as it is not modified in place."""
    # Parameters are never cached: the flat Adam kernel (ign_adam_step) rewrites them through raw pointers, which does not move
    # the version counter a cache entry is validated by -- a stale bound would let a weight that has grown overflow fp16.
    param = t.is_leaf and t.requires_grad
    cached = None if param else cached_bound(t)
    if cached is not None:
        return cached
    base = None if param else getattr(t, "_base", None)
    if base is not None and (base.is_leaf and base.requires_grad):
        base = None
    if base is not None and base.numel() == t.numel():       # a reshaped view of a tensor whose producer attached a bound
        cb = cached_bound(base)
        if cb is not None:
            return cb
    if not t.is_contiguous():
        base = getattr(t, "_base", None)
        if base is not None and base.is_contiguous() and base.dtype == t.dtype and base.numel() <= 4 * t.numel():
            return tensor_bound(base)         # a strided view (q / k / v of a packed projection): the base tensor's bound bounds it
    tc = t if t.is_contiguous() else t.contiguous()
    slot = _new_slot(t.device)
    _lib.check(_lib.lib().ign_absmax(_ptr(tc), tc.numel(), _ptr(slot), _stream()), "ign_absmax")
    if not param:
        set_bound(t, slot)
    return slot


def set_bound(t, slot):
    """Attach a known magnitude bound (one-element device tensor) to `t`; see tensor_bound / cached_bound.  A reshaped view is
    looked up through its ROOT base (`view(...).reshape(...)._base` is the root, not the intermediate view), so a bound attached
    to a full-size view is attached to that root as well."""
    cap = torch.cuda.is_current_stream_capturing()
    try:
        t._ign_bound = (slot, t._version, t.data_ptr(), cap)
        base = t._base
        if base is not None and base.numel() == t.numel() and not (base.is_leaf and base.requires_grad):
            base._ign_bound = (slot, base._version, base.data_ptr(), cap)
    except Exception:
        pass
    return t


def keep_bound(out, src, factor=1.0):
    """`out` = f(src) element-wise with |f(u)| <= factor |u|: `out` inherits src's magnitude bound, if src carries one, instead of
    being scanned when a dense layer consumes it.  factor 1: ReLU, GELU.  factor <= 2 (GELU's derivative reaches 1.13) is
    covered by the headroom of the scaling: a bound b is scaled to [2^13, 2^14), fp16 represents values below 2^16, so an
    element up to 4 b neither overflows nor loses a bit (include/ign_abi.h, "h3")."""
    cb = cached_bound(src) if factor <= 2.0 else None
    if cb is not None:
        set_bound(out, cb)
    return out


class _ActFn(torch.autograd.Function):
    """ReLU / GELU with torch's own element-wise kernels in both directions; what it adds is the magnitude bound: the output
    inherits the input's, and dL/du inherits dL/dy's (|relu'| <= 1, |gelu'| <= 1.13) -- a plain F.relu / F.gelu node hands the
    backward GEMM behind it a tensor without one, i.e. costs a pass over it (ign_absmax)."""

    @staticmethod
    def forward(ctx, u, gelu):
        ctx.gelu = gelu
        y = torch.nn.functional.gelu(u) if gelu else torch.relu(u)
        ctx.save_for_backward(u if gelu else y)
        return y

    @staticmethod
    def backward(ctx, g):
        (t,) = ctx.saved_tensors
        gu = torch.ops.aten.gelu_backward(g, t) if ctx.gelu else torch.ops.aten.threshold_backward(g, t, 0)
        return keep_bound(gu, g, 1.13 if ctx.gelu else 1.0), None


def relu(u):
    return keep_bound(_ActFn.apply(u, False), u)


def gelu(u):
    return keep_bound(_ActFn.apply(u, True), u)


# The arithmetics of a dense-layer / convolution GEMM, by the names the knobs use (GEMM_MATH, fcn.CONV_MATH): fp32 MFMA (ign_clconv_*);
# "bf16x6" (*_x6); the x6 kernels with operands rounded to bf16 and ONE product per MFMA step -- what torch.autocast(bfloat16), the
# reference's default mode, computes for a matmul; accumulation and outputs stay fp32 (*_bf16); "f16x3", which takes operand bounds (*_h3)
GEMM_F32, GEMM_X6, GEMM_BF16, GEMM_H3 = "f32", "bf16x6", "bf16", "f16x3"
WGRAD_TAPS = (2, 3, 5, 8)     # tap counts the multi-tap split weight-gradient kernels (ign_clconv_wgrad_x6 / _bf16 / _h3) exist for


def _dense_arith(autocast):
    """The arithmetic of linear / gelu_linear / conv1d_cl, of the LayerNorm bound hooks and of prepare_linear_weights: the one place
    that reads GEMM_MATH.  (The FCN body has its own knob and rule: fcn._fcn_arith.)"""
    if autocast:
        return GEMM_BF16
    return GEMM_H3 if GEMM_MATH == "f16x3" else GEMM_X6


def _linear_wgrad_split(Ci):
    """Whether a Linear layer's weight gradient runs on the split kernel (ign_linear_wgrad_*), else fp32 ign_clconv_wgrad, k = 1."""
    return Ci % 4 == 0 and LINEAR_WGRAD == "bf16x6"


def _conv_wgrad_route(k, Ci):
    """conv1d_cl's weight gradient: "split" (the multi-tap split kernel), "taps" (one Linear-layer weight gradient per tap) or
    "f32" (ign_clconv_wgrad; k = 1 goes there too)."""
    if LINEAR_WGRAD != "bf16x6":
        return "f32"
    if k in WGRAD_TAPS:
        return "split"
    return "taps" if k > 1 and Ci % 4 == 0 else "f32"


# One launcher per GEMM kind and its entry point per arithmetic.  `dims` = (B, Tin, Ci, Co, k) as the entry point takes them; the two
# operand bounds are device pointers (ctypes.c_void_p) and reach the kernel under GEMM_H3 only: otherwise callers pass None.
_CLCONV_FWD = {GEMM_F32: "ign_clconv_fwd", GEMM_X6: "ign_clconv_fwd_x6", GEMM_BF16: "ign_clconv_fwd_bf16", GEMM_H3: "ign_clconv_fwd_h3"}
_CLCONV_DGRAD = {GEMM_F32: "ign_clconv_dgrad", GEMM_X6: "ign_clconv_dgrad_x6", GEMM_BF16: "ign_clconv_dgrad_bf16",
                 GEMM_H3: "ign_clconv_dgrad_h3"}
_CLCONV_DGRAD_INPUT = {GEMM_F32: "ign_clconv_dgrad_input", GEMM_X6: "ign_clconv_dgrad_input_x6", GEMM_BF16: "ign_clconv_dgrad_input_bf16",
                       GEMM_H3: "ign_clconv_dgrad_input_h3"}
_CLCONV_WGRAD = {GEMM_F32: "ign_clconv_wgrad", GEMM_X6: "ign_clconv_wgrad_x6", GEMM_BF16: "ign_clconv_wgrad_bf16",
                 GEMM_H3: "ign_clconv_wgrad_h3"}
_LINEAR_WGRAD = {GEMM_X6: "ign_linear_wgrad_x6", GEMM_BF16: "ign_linear_wgrad_bf16", GEMM_H3: "ign_linear_wgrad_h3"}


def _clconv_fwd(arith, x, wt, bias, pro_a, pro_b, y, part, dims, b_in=None, b_w=None, amax=None):
    """y = conv(relu(pro_a x + pro_b), packed weights wt) + bias, BatchNorm partial sums into `part`: the forward of a convolution
    / dense layer, and every input gradient computed as a forward GEMM on the transposed weights.  `amax` (GEMM_H3): a slot the
    epilogue maxes max |y| into."""
    name, tail = _CLCONV_FWD[arith], ()
    if arith == GEMM_H3:
        name, tail = (name, (b_in, b_w)) if amax is None else ("ign_clconv_fwd_h3_amax", (b_in, b_w, _ptr(amax)))
    _lib.check(getattr(_lib.lib(), name)(_ptr(x), _ptr(wt), _ptr(bias), _ptr(pro_a), _ptr(pro_b), _ptr(y), _ptr(part), *tail, *dims,
                                         _stream()), name)


def _clconv_dgrad(arith, dyp, wd, y_in, a_in, b_in, mean_in, invstd_in, g_in, part, dims, b_dy=None, b_w=None):
    """The FCN body's data gradient with the BatchNorm-backward epilogue of the block below."""
    name, tail = _CLCONV_DGRAD[arith], ((b_dy, b_w) if arith == GEMM_H3 else ())
    _lib.check(getattr(_lib.lib(), name)(_ptr(dyp), _ptr(wd), _ptr(y_in), _ptr(a_in), _ptr(b_in), _ptr(mean_in), _ptr(invstd_in),
                                         _ptr(g_in), _ptr(part), *tail, *dims, _stream()), name)


def _clconv_dgrad_input(arith, dyp, wd, gx, dims, b_dy=None, b_w=None):
    """The FCN body's data gradient into the raw input series (no block below: plain epilogue), gx (B, Tin, Ci) for any Ci."""
    name, tail = _CLCONV_DGRAD_INPUT[arith], ((b_dy, b_w) if arith == GEMM_H3 else ())
    _lib.check(getattr(_lib.lib(), name)(_ptr(dyp), _ptr(wd), _ptr(gx), *tail, *dims, _stream()), name)


def _wgrad_workspace(arith, dims, device):
    """The workspace of a weight-gradient launch (_clconv_wgrad, or _linear_wgrad with dims (1, M, Ci, Co, 1))."""
    size = "ign_clconv_wgrad_workspace_bytes" if arith == GEMM_F32 else "ign_clconv_wgrad_x6_workspace_bytes"
    return torch.empty(max(1, int(getattr(_lib.lib(), size)(*dims)) // 4), device=device, dtype=torch.float32)


def _clconv_wgrad(arith, dyp, dy_pad, x, pro_a, pro_b, dw, dims, b_dy=None, b_x=None):
    """dW of a convolution from dy (zero-padded by dy_pad rows per side) and relu(pro_a x + pro_b).  dw None (split kernels): the
    partial slabs stay in the workspace for ign_clconv_wgrad_reduce_multi.  -> the workspace."""
    name, tail = _CLCONV_WGRAD[arith], ((b_dy, b_x) if arith == GEMM_H3 else ())
    ws = _wgrad_workspace(arith, dims, dyp.device)
    _lib.check(getattr(_lib.lib(), name)(_ptr(dyp), dy_pad, _ptr(x), _ptr(pro_a), _ptr(pro_b), _ptr(dw), _ptr(ws), *tail, *dims,
                                         _stream()), name)
    return ws


def _linear_wgrad(arith, dy, x, dw, db, M, Ci, Co, b_dy=None, b_x=None, ws=None):
    """dW = dy^T x and (db not None) the bias gradient in one pass over dy (M, Co) and x (M, Ci), on the split kernels.  `ws`: a
    workspace of (1, M', Ci, Co, 1), M' >= M, to reuse (the per-tap route of conv1d_cl)."""
    name, tail = _LINEAR_WGRAD[arith], ((b_dy, b_x) if arith == GEMM_H3 else ())
    if ws is None:
        ws = _wgrad_workspace(arith, (1, M, Ci, Co, 1), dy.device)
    _lib.check(getattr(_lib.lib(), name)(_ptr(dy), _ptr(x), _ptr(dw), _ptr(db), _ptr(ws), *tail, M, Ci, Co, _stream()), name)


def _pack_weights(arith, w, need_dx, b_w=None):
    """One layer's weights w (Co, Ci[, k]) in the layout the GEMMs of `arith` read: -> (forward form, transposed tap-reversed form
    for the input gradient or None).  b_w (GEMM_H3): the weight's magnitude bound, a one-element device tensor."""
    L = _lib.lib()
    Co, Ci = w.shape[:2]
    k = w.shape[2] if w.dim() == 3 else 1
    if arith == GEMM_F32:
        wt = torch.empty(Co, k * Ci, device=w.device, dtype=torch.float32)
        wd = torch.empty(Ci, k * Co, device=w.device, dtype=torch.float32) if need_dx else None
    else:
        wt = torch.empty(int(L.ign_clconv_x3_elems(Co, Ci, k)), device=w.device, dtype=torch.bfloat16)
        wd = torch.empty(int(L.ign_clconv_x3_elems(Ci, Co, k)), device=w.device, dtype=torch.bfloat16) if need_dx else None
    if arith == GEMM_H3:
        (v1, i1), name = _tables(1), "ign_clconv_pack_weights_h2_multi"
        rc = L.ign_clconv_pack_weights_h2_multi(1, v1(w.data_ptr()), v1(wt.data_ptr()), v1(wd.data_ptr()) if need_dx else None,
                                                i1(Co), i1(Ci), i1(k), None, v1(b_w.data_ptr()), _stream())
    else:
        name = "ign_clconv_pack_weights" if arith == GEMM_F32 else "ign_clconv_pack_weights_x3"
        rc = getattr(L, name)(_ptr(w), _ptr(wt), _ptr(wd), Co, Ci, k, _stream())
    _lib.check(rc, name)
    return wt, wd


_PREPARED = {}          # (data_ptr, shape) -> (w, version, generation, bound slot, packed forward planes, packed transposed planes)


def prepare_linear_weights(weights, need_dx=True):
    """Model-level prologue of the fp16-plane dense layers: the magnitude bounds of ALL the given weight matrices in one launch
    (ign_absmax_multi) and their packed plane forms in one launch per eight (ign_clconv_pack_weights_h2_multi), instead of one
    scan + one packing launch per layer.  `ops.linear` consumes the entry of its weight (once; an entry is valid only for the
    parameter values it was made from: tensor version and _lib.PARAM_GENERATION).  No-op outside the f16x3 arithmetic."""
    _PREPARED.clear()
    if _dense_arith(torch.is_autocast_enabled()) != GEMM_H3:
        return
    ws = []
    for w in weights:
        if w is None or not w.is_cuda or w.dtype != torch.float32 or w.dim() != 2 or w.shape[0] % 4 or not w.is_contiguous():
            continue
        ws.append(w)
    if not ws:
        return
    L = _lib.lib()
    dev = ws[0].device
    slots = [_new_slot(dev) for _ in ws]
    for c0 in range(0, len(ws), 16):
        cw, cs = ws[c0:c0 + 16], slots[c0:c0 + 16]
        n = len(cw)
        vpa, lla = ctypes.c_void_p * n, ctypes.c_longlong * n
        _lib.check(L.ign_absmax_multi(n, vpa(*[w.data_ptr() for w in cw]), lla(*[w.numel() for w in cw]),
                                      vpa(*[t.data_ptr() for t in cs]), _stream()), "ign_absmax_multi")
    gen = _lib.PARAM_GENERATION[0]
    for c0 in range(0, len(ws), 8):
        cw, cs = ws[c0:c0 + 8], slots[c0:c0 + 8]
        n = len(cw)
        vpa, ia = ctypes.c_void_p * n, ctypes.c_int * n
        wt = [torch.empty(int(L.ign_clconv_x3_elems(w.shape[0], w.shape[1], 1)), device=dev, dtype=torch.bfloat16) for w in cw]
        wd = [torch.empty(int(L.ign_clconv_x3_elems(w.shape[1], w.shape[0], 1)), device=dev, dtype=torch.bfloat16) if need_dx else None
              for w in cw]
        _lib.check(L.ign_clconv_pack_weights_h2_multi(n, vpa(*[w.data_ptr() for w in cw]), vpa(*[t.data_ptr() for t in wt]),
                                                      vpa(*[(t.data_ptr() if t is not None else None) for t in wd]) if need_dx else None,
                                                      ia(*[w.shape[0] for w in cw]), ia(*[w.shape[1] for w in cw]), ia(*([1] * n)), None,
                                                      vpa(*[t.data_ptr() for t in cs]), _stream()), "ign_clconv_pack_weights_h2_multi")
        for w, sl, a, b in zip(cw, cs, wt, wd):
            _PREPARED[(w.data_ptr(), tuple(w.shape))] = (w, w._version, gen, sl, a, b)


def _take_prepared(w, need_dx):
    ent = _PREPARED.pop((w.data_ptr(), tuple(w.shape)), None)
    if ent is None or ent[1] != w._version or ent[2] != _lib.PARAM_GENERATION[0] or (need_dx and ent[5] is None):
        return None
    return ent


def _linear_forward(ctx, x, w, bias, extra=()):
    """LinearFn.forward; `extra`: tensors saved behind x2 (GeluLinearFn: the pre-activation)."""
    Co, Ci = w.shape
    x2 = x.reshape(-1, Ci)
    x2 = x2 if x2.is_contiguous() else x2.contiguous()
    M = x2.shape[0]
    w = w.contiguous()
    dev = x.device
    need_dx = ctx.needs_input_grad[0]
    arith = ctx.arith = _dense_arith(torch.is_autocast_enabled())
    y = torch.empty(*x.shape[:-1], Co, device=dev, dtype=torch.float32)    # final shape (not a view: its reshaped views find its bound)
    ctx.bx = ctx.bw = prepared = None
    if arith == GEMM_H3:
        # operand bounds on the device (the input's is inherited from x when x2 is a view); the weight's bound and packed planes
        # come from the model's prologue launch (prepare_linear_weights) where there was one
        ctx.bx = tensor_bound(x) if x2.data_ptr() == x.data_ptr() and x.is_contiguous() else tensor_bound(x2)
        prepared = _take_prepared(w, need_dx)
        ctx.bw = prepared[3] if prepared is not None else tensor_bound(w)
    wt3, wd3 = (prepared[4], prepared[5] if need_dx else None) if prepared is not None else _pack_weights(arith, w, need_dx, ctx.bw)
    # the epilogue also takes max |y|: the operand bound of whatever dense layer / attention core consumes y
    yb = _new_slot(dev) if arith == GEMM_H3 else None
    _clconv_fwd(arith, x2, wt3, bias, None, None, y, None, (1, M, Ci, Co, 1), _ptr(ctx.bx), _ptr(ctx.bw), yb)
    ctx.save_for_backward(x2, *extra)
    ctx.wd3, ctx.dims, ctx.has_bias, ctx.xshape = wd3, (M, Ci, Co), bias is not None, x.shape
    ctx.mark_non_differentiable(*([yb] if yb is not None else []))
    ctx.set_materialize_grads(False)              # no zero-filled "gradient" of the bound output per backward call
    return y, yb


def _linear_backward(ctx, gy, gelu=False):
    """LinearFn.backward.  `gelu`: the layer's input was gelu(u), u saved behind x2 -- the returned input gradient is dL/du, the
    activation's derivative applied in the epilogue of the input-gradient GEMM (ign_linear_dgrad_gelu_h3) where the shape allows."""
    if gy is None:
        return None, None, None
    x2 = ctx.saved_tensors[0]
    u2 = ctx.saved_tensors[1].reshape(x2.shape) if gelu else None
    M, Ci, Co = ctx.dims
    g2 = gy.reshape(M, Co)
    g2 = g2 if g2.is_contiguous() else g2.contiguous()
    dx = dw = db = None
    arith = ctx.arith
    bg = tensor_bound(g2) if arith == GEMM_H3 else None
    if ctx.needs_input_grad[0]:
        dx = torch.empty(M, Ci, device=g2.device, dtype=torch.float32)
        dxb = _new_slot(g2.device) if arith == GEMM_H3 else None     # the epilogue takes max |dx|: the next backward GEMM's bound
        fused = gelu and arith == GEMM_H3 and Ci % 256 == 0 and Co % 4 == 0 and u2.is_contiguous()
        if fused:                                # dL/du = (g W) * gelu'(u) in one GEMM
            _lib.check(_lib.lib().ign_linear_dgrad_gelu_h3(_ptr(g2), _ptr(ctx.wd3), _ptr(u2), _ptr(dx), _ptr(bg), _ptr(ctx.bw),
                                                           _ptr(dxb), M, Co, Ci, _stream()), "ign_linear_dgrad_gelu_h3")
        else:
            _clconv_fwd(arith, g2, ctx.wd3, None, None, None, dx, None, (1, M, Co, Ci, 1), _ptr(bg), _ptr(ctx.bw), dxb)
        if gelu and not fused:                   # shapes / arithmetics outside the fused kernel: torch's element-wise backward
            dx = torch.ops.aten.gelu_backward(dx, u2)     # (|gelu'| <= 1.13: dxb stays a usable bound, see keep_bound)
        dx = dx.view(ctx.xshape)
        if dxb is not None:
            set_bound(dx, dxb)
    want_db = ctx.has_bias and ctx.needs_input_grad[2]
    if ctx.needs_input_grad[1]:
        dw = torch.empty(Co, Ci, device=g2.device, dtype=torch.float32)
        if _linear_wgrad_split(Ci):
            # weight and bias gradient in one pass over dy (the bias gradient rides on the tiles that stage dy anyway)
            if want_db:
                db = torch.empty(Co, device=g2.device, dtype=torch.float32)
            _linear_wgrad(arith, g2, x2, dw, db, M, Ci, Co, _ptr(bg), _ptr(ctx.bx))
        else:
            _clconv_wgrad(GEMM_F32, g2, 0, x2, None, None, dw, (1, M, Ci, Co, 1))
    if want_db and db is None:
        db = g2.sum(dim=0)
    return dx, dw, db


class LinearFn(torch.autograd.Function):
    """y = x W^T + b for the dense layers of the two encoder baselines (IGN/layers/SelfAttention_Family.py:195-211,
    IGN/layers/Transformer_EncDec.py:33-48, nn.TransformerEncoderLayer in IGN/model/eegcnn.py:219-228) on the library's own
    GEMM kernels instead of hipBLASLt: a Linear layer is the k = 1 case of the channels-last convolution, so forward and the
    input gradient run on the split-bf16 kernel (fp32 accuracy on the bf16 matrix cores, ign_clconv_fwd_x6 with the weight
    resp. its transpose), and so does the weight gradient (ign_clconv_wgrad_x6, k = 1: 128 x 128 tiles, transposing LDS reads);
    `LINEAR_WGRAD = "f32"` (tests) keeps it on the fp32-MFMA TN kernel (ign_clconv_wgrad)."""

    @staticmethod
    def forward(ctx, x, w, bias):
        return _linear_forward(ctx, x, w, bias)

    @staticmethod
    def backward(ctx, gy, _gyb=None):
        return _linear_backward(ctx, gy)


class GeluLinearFn(torch.autograd.Function):
    """z = gelu(u) W^T + b -- the activation and second dense layer of an encoder's feed-forward block
    (IGN/layers/Transformer_EncDec.py:46-47) as one node: forward = torch's GELU kernel + the dense layer's GEMM; backward = the
    weight gradient from the saved gelu(u) and the input gradient THROUGH the activation in one GEMM (ign_linear_dgrad_gelu_h3:
    dL/dy is never written, aten::gelu_backward's three passes over the (rows, d_ff) tensors disappear)."""

    @staticmethod
    def forward(ctx, u, w, bias):
        y = keep_bound(torch.nn.functional.gelu(u), u)
        return _linear_forward(ctx, y, w, bias, extra=(u,))

    @staticmethod
    def backward(ctx, gy, _gyb=None):
        return _linear_backward(ctx, gy, gelu=True)


def linear(x, w, bias=None):
    """nn.Linear / 1x1 Conv1d on the hand-written GEMM kernels (inside an autocast region: their single-product bf16 form);
    shapes they do not cover (and non-fp32 tensors) go to torch's GEMM."""
    if not x.is_cuda:
        raise _lib.IgnError(f"linear: tensor on {x.device}; the product path runs on the MI355X only (no CPU fallback)")
    if (x.dtype != torch.float32 or w.dtype != torch.float32
            or w.shape[0] % 4 or x.numel() == 0 or x.shape[-1] != w.shape[1]
            or x.numel() // x.shape[-1] >= (1 << 30)):
        return torch.nn.functional.linear(x, w, bias)
    y, yb = LinearFn.apply(x, w, bias)
    if yb is not None:
        set_bound(y, yb)
    return y


def gelu_linear(u, w, bias=None):
    """linear(gelu(u), w, bias) with the GELU's backward folded into the dense layer's input-gradient GEMM (GeluLinearFn); inputs the
    hand-written GEMMs do not cover take the two-op route."""
    if (not u.is_cuda or u.dtype != torch.float32 or w.dtype != torch.float32 or w.shape[0] % 4 or u.numel() == 0
            or u.shape[-1] != w.shape[1] or u.numel() // u.shape[-1] >= (1 << 30)):
        return linear(gelu(u), w, bias)
    y, yb = GeluLinearFn.apply(u, w, bias)
    if yb is not None:
        set_bound(y, yb)
    return y


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm over the last dimension on ign_layernorm_fwd / _bwd (HBM-bound row kernels; torch's kernels for narrow rows
    -- PatchTST's 3.9 M rows of 64 -- run 10x off the memory roofline)."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, eps):
        """`res` (same shape as x, or None): the row normalised is x + res -- the residual connection of a post-norm encoder
        layer -- added inside the same pass (ign_layernorm_res_fwd)."""
        _need_gpu("layer_norm", x, res, weight, bias)
        L = _lib.lib()
        D = x.shape[-1]
        x2 = x.reshape(-1, D)
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        R = x2.shape[0]
        y = torch.empty_like(x2)
        mean = torch.empty(R, device=x.device, dtype=torch.float32)
        rstd = torch.empty(R, device=x.device, dtype=torch.float32)
        if res is not None:
            r2 = res.reshape(-1, D)
            r2 = r2 if r2.is_contiguous() else r2.contiguous()
            if r2.shape != x2.shape:
                raise _lib.IgnError(f"layer_norm: residual {tuple(res.shape)} does not match {tuple(x.shape)}")
            s2 = torch.empty_like(x2)
            _lib.check(L.ign_layernorm_res_fwd(_ptr(x2), _ptr(r2), _ptr(s2), _ptr(weight), _ptr(bias), _ptr(y), _ptr(mean), _ptr(rstd),
                                               R, D, float(eps), _stream()), "ign_layernorm_res_fwd")
            x2 = s2
        else:
            _lib.check(L.ign_layernorm_fwd(_ptr(x2), _ptr(weight), _ptr(bias), _ptr(y), _ptr(mean), _ptr(rstd), R, D, float(eps),
                                           _stream()), "ign_layernorm_fwd")
        ctx.save_for_backward(x2, weight, mean, rstd)
        ctx.has_bias = bias is not None
        ctx.has_res = res is not None
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        x2, weight, mean, rstd = ctx.saved_tensors
        R, D = x2.shape
        g2 = gy.reshape(R, D)
        g2 = g2 if g2.is_contiguous() else g2.contiguous()
        gx = torch.empty_like(x2)
        need_w = ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3])
        dgamma = torch.empty(D, device=x2.device, dtype=torch.float32) if need_w else None
        dbeta = torch.empty(D, device=x2.device, dtype=torch.float32) if need_w and ctx.has_bias else None
        part = torch.empty(int(L.ign_layernorm_parts(R, D)) * 2 * D, device=x2.device, dtype=torch.float32)
        gxv = gx.view(gy.shape)
        if _dense_arith(torch.is_autocast_enabled()) == GEMM_H3:
            # dL/dx usually feeds the backward GEMMs of a dense layer: its magnitude bound is taken here, as it is written
            slot = _new_slot(x2.device)
            _lib.check(L.ign_layernorm_bwd_amax(_ptr(x2), _ptr(g2), _ptr(weight), _ptr(mean), _ptr(rstd), _ptr(gx), _ptr(dgamma),
                                                _ptr(dbeta), _ptr(part), _ptr(slot), R, D, _stream()), "ign_layernorm_bwd_amax")
            set_bound(gxv, slot)
        else:
            _lib.check(L.ign_layernorm_bwd(_ptr(x2), _ptr(g2), _ptr(weight), _ptr(mean), _ptr(rstd), _ptr(gx), _ptr(dgamma), _ptr(dbeta),
                                           _ptr(part), R, D, _stream()), "ign_layernorm_bwd")
        return gxv, (gxv if ctx.has_res else None), dgamma, dbeta, None          # d(x + res): the same gradient for both addends


def layer_norm(x, norm, residual=None):
    """Apply an nn.LayerNorm module (normalised over the last dimension, affine) on the hand-written kernels; shapes they do not
    cover go through the module itself (torch on the GPU).  `residual`: normalise x + residual (the add rides on the same pass)."""
    D = x.shape[-1]
    # torch's kernels fall off the memory roofline for many narrow rows (Transformer: 256 000 rows of 512, 96.9 -> 94.9 ms/step;
    # PatchTST: 3.9 M rows of 64, 123.9 -> 79.4 ms/step); for few rows (EEG-CNN: 25 600 rows of 512) the grid is sized by the row
    # count and the d(gamma) partials are reduced in parallel: 22 / 37 us per call against torch's 34 / 97 (7.52 -> 7.36 ms/step)
    if (not x.is_cuda or x.dtype != torch.float32 or norm.weight is None or len(norm.normalized_shape) != 1 or D % 4 or D > 2048
            or x.numel() == 0 or x.numel() < LAYERNORM_MIN_ROWS * D
            or (residual is not None and (residual.shape != x.shape or residual.dtype != x.dtype or not residual.is_cuda))):
        return norm(x if residual is None else x + residual)
    out = LayerNormFn.apply(x, residual, norm.weight, norm.bias, norm.eps)
    if norm.bias is not None and _dense_arith(torch.is_autocast_enabled()) == GEMM_H3:
        # a row standardised with its own mean and (biased) variance over D elements cannot exceed sqrt(D - 1): the output is
        # bounded by max_d(|gamma_d| sqrt(D - 1) + |beta_d|) -- from the parameters alone, one tiny launch instead of a pass over
        # the activations when a dense layer behind it asks for its operand's magnitude (tensor_bound)
        slots = torch.empty(4, device=x.device, dtype=torch.float32)
        v1, i1, l1 = ctypes.c_void_p * 1, ctypes.c_int * 1, ctypes.c_longlong * 1
        wp, bp = norm.weight.data_ptr(), norm.bias.data_ptr()
        _lib.check(_lib.lib().ign_fcn_scan(1, v1(wp), l1(D), v1(wp), v1(bp), i1(D), l1(max(D, 2)), _ptr(slots), None, 0, _stream()), "ign_fcn_scan")
        set_bound(out, slots[1:2])
    return out


class ConvCLFn(torch.autograd.Function):
    """Valid, stride-1 Conv1d on a CHANNELS-LAST tensor: x (B, Tin, Ci), w (Co, Ci, k) -> y (B, Tin-k+1, Co).

    The general-purpose door to the implicit-GEMM kernels of the FCN expert (csrc/ign_clconv_x6.hip) for the other deep
    experts and embeddings (IGN/model/ResNet.py:11-22,46; IGN/layers/Embed.py:32-36): padding is materialised by the caller
    (zero rows, circular rows), a strided convolution is a stride-1 one over a space-to-depth view.  Forward and input
    gradient run on ign_clconv_fwd_x6 (the latter on dy zero-padded by k-1 rows with the tap-reversed transposed weights),
    the weight gradient on ign_clconv_wgrad_x6 where its tap count is instantiated (k in 2,3,5,8), on one ign_linear_wgrad_x6 per tap
    for the other k > 1 with Ci % 4 == 0, else (k = 1 included) on the fp32-MFMA ign_clconv_wgrad: _conv_wgrad_route.  Each in the
    arithmetic of _dense_arith."""

    @staticmethod
    def forward(ctx, x, w, bias):
        _need_gpu("conv1d_cl", x, w)
        B, Tin, Ci = x.shape
        Co, Ci2, k = w.shape
        if Ci2 != Ci or Tin < k or Co % 4:
            raise _lib.IgnError(f"conv1d_cl: x {tuple(x.shape)} / w {tuple(w.shape)}: needs matching channels, Tin >= k, Co % 4 == 0")
        x = x.contiguous()
        w = w.contiguous()
        y = torch.empty(B, Tin - k + 1, Co, device=x.device, dtype=torch.float32)
        arith = ctx.arith = _dense_arith(torch.is_autocast_enabled())
        ctx.bx = ctx.bw = None
        if arith == GEMM_H3:
            ctx.bw, ctx.bx = tensor_bound(w), tensor_bound(x)
        wt3, wd3 = _pack_weights(arith, w, ctx.needs_input_grad[0], ctx.bw)
        _clconv_fwd(arith, x, wt3, bias, None, None, y, None, (B, Tin, Ci, Co, k), _ptr(ctx.bx), _ptr(ctx.bw))
        ctx.save_for_backward(x)
        ctx.wd3, ctx.dims, ctx.has_bias = wd3, (B, Tin, Ci, Co, k), bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        B, Tin, Ci, Co, k = ctx.dims
        Tout = Tin - k + 1
        dx = dw = db = None
        # dy zero-padded by k-1 rows per side: the operand of the input gradient, and the layout the weight gradient reads
        gyp = torch.nn.functional.pad(gy, (0, 0, k - 1, k - 1)) if k > 1 else gy.contiguous()
        arith = ctx.arith
        bg = tensor_bound(gyp) if arith == GEMM_H3 else None  # (the zero rows do not change the maximum)
        if ctx.needs_input_grad[0]:
            dx = torch.empty(B, Tin, Ci, device=gy.device, dtype=torch.float32)
            _clconv_fwd(arith, gyp, ctx.wd3, None, None, None, dx, None, (B, Tout + 2 * (k - 1), Co, Ci, k), _ptr(bg), _ptr(ctx.bw))
        if ctx.needs_input_grad[1]:
            route = _conv_wgrad_route(k, Ci)
            if route == "taps":
                # tap counts without an instantiated multi-tap kernel (k = 4, 7, 11, ...): one k = 1 GEMM per tap on FLAT row
                # views.  With dy zero-padded by k-1 rows at the END of every sample, dW[:, :, j] = dy_flat[0 : M-j]^T x_flat[j : M]
                # -- the pairs that straddle two samples multiply zero rows -- so each tap is the Linear-layer weight gradient
                # on the split kernel with the operand advanced by j rows (no copies of x).
                M = B * Tin
                dye = torch.nn.functional.pad(gy, (0, 0, 0, k - 1)).contiguous()
                dwt = torch.empty(k, Co, Ci, device=gy.device, dtype=torch.float32)
                ws = _wgrad_workspace(arith, (1, M, Ci, Co, 1), gy.device)
                xf = x.view(M, Ci)
                for j in range(k):
                    _linear_wgrad(arith, dye, xf[j:], dwt[j], None, M - j, Ci, Co, _ptr(bg), _ptr(ctx.bx), ws)
                dw = dwt.permute(1, 2, 0).contiguous()
            else:
                dw = torch.empty(Co, Ci, k, device=gy.device, dtype=torch.float32)
                _clconv_wgrad(arith if route == "split" else GEMM_F32, gyp, k - 1, x, None, None, dw, (B, Tin, Ci, Co, k), _ptr(bg),
                              _ptr(ctx.bx))
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = gy.sum(dim=(0, 1))
        return dx, dw, db


def conv1d_cl(x_btc, w_oik, bias=None):
    """Valid stride-1 Conv1d over (B, T, C) channels-last input on the hand-written kernels (see ConvCLFn)."""
    return ConvCLFn.apply(x_btc, w_oik, bias)


class GiniGateFn(torch.autograd.Function):
    """(sbm_out, dnn_out) -> (mixture, eta); IGN/model/InterpGN.py:44-52."""

    @staticmethod
    def forward(ctx, sbm, dnn, gating_value):
        _need_gpu("gini_gate", sbm, dnn)
        sbm, dnn = sbm.contiguous(), dnn.contiguous()
        B, N = sbm.shape
        out = torch.empty_like(sbm)
        eta = torch.empty(B, 1, device=sbm.device, dtype=torch.float32)
        use, gv = (0, 0.0) if gating_value is None else (1, float(gating_value))
        _lib.check(_lib.lib().ign_gate_fwd(_ptr(sbm), _ptr(dnn), _ptr(out), _ptr(eta), B, N, gv, use, _stream()), "ign_gate_fwd")
        ctx.save_for_backward(sbm, dnn)
        ctx.gv = (use, gv)
        ctx.set_materialize_grads(False)              # eta usually carries no gradient: no zero fill for it
        return out, eta

    @staticmethod
    def backward(ctx, gout, geta):
        sbm, dnn = ctx.saved_tensors
        B, N = sbm.shape
        use, gv = ctx.gv
        gs, gd = torch.empty_like(sbm), torch.empty_like(dnn)
        if gout is None and geta is None:
            return None, None, None
        gout = torch.zeros_like(sbm) if gout is None else gout
        geta = geta.contiguous() if geta is not None else None
        _lib.check(_lib.lib().ign_gate_bwd(_ptr(sbm), _ptr(dnn), _ptr(gout.contiguous()), _ptr(geta), _ptr(gs), _ptr(gd), B, N,
                                           gv, use, _stream()), "ign_gate_bwd")
        return gs, gd, None


def gini_gate(sbm_out, dnn_out, gating_value=None):
    return GiniGateFn.apply(sbm_out.float(), dnn_out.float(), gating_value)


_UNIT = {}


def unit_grad(device):
    """The constant 1.0 on `device` (one cached 0-dim tensor): the root gradient of `backward(loss)`."""
    t = _UNIT.get(device)
    if t is None:
        t = _UNIT[device] = torch.ones((), device=device, dtype=torch.float32)
    return t


def backward(loss):
    """loss.backward() without the two launches autograd spends on the root of the graph: `ones_like(loss)` is replaced by a
    cached constant, and ops.ign_loss recognises that constant (by address) and hands out its saved logit gradients unscaled."""
    if loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32:
        loss.backward(gradient=unit_grad(loss.device))
    else:
        loss.backward()


def _loss_tail(entry, sbm, dnn, crit, beta, reg, rule=None, more=()):
    """The one launcher of the gated loss tails -> (loss3, out, eta, gsd): loss3[2] = criterion(gate(sbm, dnn)) + beta*criterion(sbm)
    [+ reg], gsd (2, B, N) = its gradient w.r.t. (sbm, dnn) in one buffer.  `entry`: "ign_loss" (cross-entropy; by label `rule`:
    None, crit = (labels,) | "weighted", also label-smoothed, crit = (labels, class weights or None), more = (label_smoothing,) |
    "soft", the same with soft labels, crit = (labels, second labels, lam, class weights or None), more = (label_smoothing,)) or
    "ign_crps_loss" (CRPS, crit = (target, edges)); `crit` sits between `dnn` and `reg` in the entry point's signature, the numbers
    `more` between `beta` and the stream."""
    symbol = {("ign_loss", None): "ign_loss_fwd_bwd_reg", ("ign_loss", "weighted"): "ign_loss_w_fwd_bwd_reg",
              ("ign_loss", "soft"): "ign_loss_mix_fwd_bwd_reg", ("ign_crps_loss", None): "ign_loss_crps_fwd_bwd_reg"}[entry, rule]
    B, N = sbm.shape
    out = torch.empty_like(sbm)
    gsd = torch.empty(2, B, N, device=sbm.device, dtype=torch.float32)
    eta = torch.empty(B, 1, device=sbm.device, dtype=torch.float32)
    loss3 = torch.empty(3, device=sbm.device, dtype=torch.float32)
    if reg is not None:
        reg = reg.contiguous().reshape(-1)
        if reg.numel() != 1:
            raise _lib.IgnError(f"{entry}: the regulariser must be one value, got {tuple(reg.shape)}")
    _lib.check(getattr(_lib.lib(), symbol)(_ptr(sbm), _ptr(dnn), *map(_ptr, crit), _ptr(reg), _ptr(out), _ptr(eta), _ptr(loss3),
                                           _ptr(gsd[0]), _ptr(gsd[1]), B, N, float(beta), *more, _stream()), symbol)
    return loss3, out, eta, gsd


def _tail_forward(ctx, entry, sbm, dnn, prepare, crit, beta, reg, rule=None, more=()):
    """What the forwards of IgnLossFn and IgnCrpsLossFn share -> (loss, out, eta); out / eta are reporting outputs.  `prepare`
    (_ce_inputs / _crps_inputs) checks the node's criterion arguments `crit` against the (B, N) logits and converts them; `rule` and
    `more` are _loss_tail's."""
    _need_gpu(entry, sbm, dnn, reg)
    sbm, dnn = sbm.contiguous(), dnn.contiguous()
    if dnn.shape != sbm.shape:                        # the kernel reads B*N elements of each
        raise _lib.IgnError(f"{entry}: expert logits {tuple(sbm.shape)} vs {tuple(dnn.shape)}")
    loss3, out, eta, gsd = _loss_tail(entry, sbm, dnn, prepare(entry, sbm, *crit), beta, reg, rule, more)
    ctx.save_for_backward(gsd)
    ctx.n_crit, ctx.has_reg = len(crit), reg is not None
    ctx.mark_non_differentiable(out, eta)
    ctx.set_materialize_grads(False)              # no zero-filled "gradients" of the two reporting outputs per step
    return loss3[2], out, eta


def _tail_backward(ctx, gl):
    """-> (gsbm, gdnn, None per criterion argument and for beta, greg = the root gradient, passed through)."""
    if gl is None:
        return (None,) * (ctx.n_crit + 4)
    g = _unit_or_scaled(gl, ctx.saved_tensors[0])     # the root of ops.backward(): exactly 1 -- no scaling launch; else one for both
    return (g[0], g[1], *(None,) * (ctx.n_crit + 1), gl.reshape(1) if ctx.has_reg else None)


def _ce_inputs(name, logits, y):
    _check_classes(name, logits.shape[1])
    return (y.contiguous().long(),)


class IgnLossFn(torch.autograd.Function):
    """CE(gate(sbm, dnn), y) + beta * CE(sbm, y) [+ reg] with both logit gradients from one launch (_loss_tail).  The optional
    `opts` = (class_weight, label_smoothing) after `reg` select the weighted / label-smoothed tail, (class_weight, label_smoothing,
    y_b, lam) the soft-label tail of mixup / CutMix; they carry no gradient."""

    @staticmethod
    def forward(ctx, sbm, dnn, y, beta, reg, *opts):
        ctx.n_opts = len(opts)
        class_weight, label_smoothing, *soft = opts or (None, 0.0)
        if soft:                                      # (y_b, lam)
            rule, extra = "soft", (soft[0].contiguous().long(), soft[1], class_weight)
        elif class_weight is None and label_smoothing == 0.0:
            rule, extra = None, ()
        else:
            rule, extra = "weighted", (class_weight,)
        return _tail_forward(ctx, "ign_loss", sbm, dnn, lambda name, logits, y: _ce_inputs(name, logits, y) + extra, (y,), beta, reg,
                             rule, (float(label_smoothing),) if rule else ())

    @staticmethod
    def backward(ctx, gl, gout, geta):
        return _tail_backward(ctx, gl) + (None,) * ctx.n_opts


def _check_ce_options(name, logits, class_weight, label_smoothing):
    """The host's refusals of ign_loss's options, before any device work.  The VALUES of the weights (positive, finite) are the
    caller's to check where it builds them (utils.class_weight.check_weights): looking at them here would cost a sync per step."""
    if not 0.0 <= label_smoothing < 1.0:
        raise _lib.IgnError(f"{name}: label_smoothing={label_smoothing} outside [0, 1)")
    if class_weight is None:
        return
    N = logits.shape[-1]
    if not (torch.is_tensor(class_weight) and class_weight.dtype == torch.float32 and tuple(class_weight.shape) == (N,)
            and class_weight.device == logits.device):
        what = (f"{class_weight.dtype} {tuple(class_weight.shape)} on {class_weight.device}" if torch.is_tensor(class_weight)
                else type(class_weight).__name__)
        raise _lib.IgnError(f"{name}: class_weight must be a float32 ({N},) tensor on {logits.device}, got {what}")


def _check_soft_labels(name, logits, y_b, lam):
    """The host's refusals of ign_loss's soft labels: y_b and lam come together, one per row, lam float32 on the logits' device.
    The VALUES of lam (in [0, 1]) are the caller's (utils.mix.mix_draws); the kernel clamps them."""
    if y_b is None or lam is None:
        raise _lib.IgnError(f"{name}: y_b and lam come together (the second label of every row and the share of the first)")
    B = logits.shape[0]
    if not (torch.is_tensor(y_b) and not y_b.dtype.is_floating_point and y_b.numel() == B and y_b.device == logits.device):
        what = f"{y_b.dtype} {tuple(y_b.shape)} on {y_b.device}" if torch.is_tensor(y_b) else type(y_b).__name__
        raise _lib.IgnError(f"{name}: y_b must hold {B} integer labels on {logits.device}, got {what}")
    if not (torch.is_tensor(lam) and lam.dtype == torch.float32 and tuple(lam.shape) == (B,) and lam.device == logits.device):
        what = f"{lam.dtype} {tuple(lam.shape)} on {lam.device}" if torch.is_tensor(lam) else type(lam).__name__
        raise _lib.IgnError(f"{name}: lam must be a float32 ({B},) tensor on {logits.device}, got {what}")
    if lam.requires_grad:
        raise _lib.IgnError(f"{name}: lam requires a gradient; the tail has none for it")


def ign_loss(sbm_out, dnn_out, y, beta=1.0, reg=None, class_weight=None, label_smoothing=0.0, y_b=None, lam=None):
    """-> (CE(mix, y) + beta*CE(sbm, y) [+ reg], mix, eta); mix / eta are reporting outputs (no gradient flows through them).
    `reg`: the model's regulariser value (ModelInfo.loss, one element) -- added on the device inside the same launch, i.e. the
    whole training loss of IGN/exp/experiment_classification.py:325-329 (its gradient passes straight through).
    `class_weight` (float32 (N,) on the logits' device, positive and finite) / `label_smoothing` (in [0, 1)): both CE terms become
    F.cross_entropy(., y, weight=class_weight, label_smoothing=label_smoothing), still one launch (ign_loss_w_fwd_bwd_reg).  Without
    them the call is today's node on today's entry point, bit for bit.
    `y_b` (integer labels (B,)) / `lam` (float32 (B,) in [0, 1], no gradient): soft labels of mixup / CutMix -- every row counts as
    class y with the share lam and as class y_b with 1 - lam in both criteria (ign_loss_mix_fwd_bwd_reg, one launch; the formula is
    utils/mix.py's CEm); lam == 1 is the call without them."""
    soft = y_b is not None or lam is not None
    opts = ()                                         # the default call: a node of five inputs
    if soft or class_weight is not None or label_smoothing != 0.0:
        _check_ce_options("ign_loss", sbm_out, class_weight, label_smoothing)
        opts = (class_weight.contiguous() if class_weight is not None else None, float(label_smoothing))
    if soft:
        _check_soft_labels("ign_loss", sbm_out, y_b, lam)
        opts += (y_b.reshape(-1), lam.contiguous())
    return IgnLossFn.apply(sbm_out.float(), dnn_out.float(), y, beta, reg, *opts)


def _crps_inputs(name, logits, target, edges):
    """-> (fp32 target (B,), fp64 edges (N,)) on the logits' device, checked against the (B, N) logits."""
    B, N = logits.shape
    _check_classes(name, N)
    target = target.reshape(-1).to(device=logits.device, dtype=torch.float32).contiguous()
    edges = edges.reshape(-1).to(device=logits.device, dtype=torch.float64).contiguous()
    if target.numel() != B or edges.numel() != N:
        raise _lib.IgnError(f"{name}: logits {tuple(logits.shape)} need {B} targets and {N} bin edges, "
                            f"got {target.numel()} and {edges.numel()}")
    return target, edges


def _unit_or_scaled(gl, g):
    """The saved logit gradient(s) handed out unscaled for the cached unit root of ops.backward(), else scaled by gl."""
    unit = _UNIT.get(gl.device)
    return g if (unit is not None and gl.data_ptr() == unit.data_ptr()) else gl * g


class CrpsLossFn(torch.autograd.Function):
    """CRPS(softmax(logits), step CDF of target) (batch mean) with its logit gradient from one launch (ign_crps_fwd_bwd)."""

    @staticmethod
    def forward(ctx, logits, target, edges):
        _need_gpu("crps_loss", logits)
        logits = logits.contiguous()
        B, N = logits.shape
        target, edges = _crps_inputs("crps_loss", logits, target, edges)
        grad = torch.empty_like(logits)
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        _lib.check(_lib.lib().ign_crps_fwd_bwd(_ptr(logits), _ptr(target), _ptr(edges), _ptr(loss), _ptr(grad), B, N, _stream()),
                   "ign_crps_fwd_bwd")
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, gl):
        (grad,) = ctx.saved_tensors
        return _unit_or_scaled(gl, grad), None, None


def crps_loss(logits, target, edges):
    """CRPSLoss of IGN/exp/experiment_regression.py:59-76: mean_b sum_j (cumsum(softmax(logits))_bj - [edges_j >= target_b])^2.
    target (B,) or (B, 1), real-valued (compared in float64, not truncated); edges (N,) with the last one +inf.  Under bf16
    autocast the logits are cast to fp32 first, as autocast does for softmax / cumsum."""
    return CrpsLossFn.apply(logits.float(), target, edges)


class IgnCrpsLossFn(torch.autograd.Function):
    """CRPS(gate(sbm, dnn)) + beta * CRPS(sbm) [+ reg] with both logit gradients from one launch (_loss_tail)."""

    @staticmethod
    def forward(ctx, sbm, dnn, target, edges, beta, reg):
        return _tail_forward(ctx, "ign_crps_loss", sbm, dnn, _crps_inputs, (target, edges), beta, reg)

    @staticmethod
    def backward(ctx, gl, gout, geta):
        return _tail_backward(ctx, gl)


def ign_crps_loss(sbm_out, dnn_out, target, edges, beta=1.0, reg=None):
    """-> (CRPS(mix) + beta*CRPS(sbm) [+ reg], mix, eta): InterpGN's regression training loss
    (IGN/exp/experiment_regression.py:159-169) in one launch; mix / eta equal ops.gini_gate's bitwise and carry no gradient.
    `reg`: the model's regulariser value (ModelInfo.loss, one element), added on the device."""
    return IgnCrpsLossFn.apply(sbm_out.float(), dnn_out.float(), target, edges, beta, reg)


class Conv1SumSqFn(torch.autograd.Function):
    """m2[f] = sum_{rows,t} ((w1[f] (*) x_row)[t] - mu[f])^2 without storing the convolution (ign_conv1_sumsq_*).
    d m2 / d mu = -2 sum (y1 - mu) = 0 when mu is the batch mean, which is the only use (BatchNorm-1 of EEG-CNN)."""

    @staticmethod
    def forward(ctx, x_rows, w1, mu, pad_left):
        _need_gpu("conv1_sumsq", x_rows, w1, mu)
        x_rows, w1, mu = x_rows.contiguous(), w1.contiguous(), mu.contiguous()
        R, T = x_rows.shape
        F1, k1 = w1.shape
        L = _lib.lib()
        ws = torch.empty(L.ign_conv1_sumsq_workspace_bytes(R, F1, k1) // 4, device=x_rows.device, dtype=torch.float32)
        m2 = torch.empty(F1, device=x_rows.device, dtype=torch.float32)
        _lib.check(L.ign_conv1_sumsq_fwd(_ptr(x_rows), _ptr(w1), _ptr(mu), _ptr(m2), _ptr(ws), R, T, F1, k1, int(pad_left),
                                         _stream()), "ign_conv1_sumsq_fwd")
        ctx.save_for_backward(x_rows, w1, mu)
        ctx.pl = int(pad_left)
        return m2

    @staticmethod
    def backward(ctx, g):
        x_rows, w1, mu = ctx.saved_tensors
        R, T = x_rows.shape
        F1, k1 = w1.shape
        L = _lib.lib()
        ws = torch.empty(L.ign_conv1_sumsq_workspace_bytes(R, F1, k1) // 4, device=x_rows.device, dtype=torch.float32)
        G = torch.empty(F1, k1, device=x_rows.device, dtype=torch.float32)
        _lib.check(L.ign_conv1_sumsq_bwd(_ptr(x_rows), _ptr(w1), _ptr(mu), _ptr(G), _ptr(ws), R, T, F1, k1, ctx.pl, _stream()),
                   "ign_conv1_sumsq_bwd")
        return None, 2.0 * g.unsqueeze(1) * G, None, None


def autocorr(x_rows, K):
    """C[d] = sum over rows and u of x[row,u] * x[row,u+d], d < K <= 128, as float64 (ign_autocorr_fwd; no gradient: the
    operand is input data)."""
    _need_gpu("autocorr", x_rows)
    L = _lib.lib()
    x_rows = x_rows.contiguous()
    R, T = x_rows.shape
    part = torch.empty(int(L.ign_autocorr_parts(R)), K, device=x_rows.device, dtype=torch.float32)
    _lib.check(L.ign_autocorr_fwd(_ptr(x_rows), _ptr(part), R, T, K, _stream()), "ign_autocorr_fwd")
    return part.sum(dim=0, dtype=torch.float64)


def edge_lagprod(x_rows, k, pad_left):
    """(Dh, Dt), float64 (k-1, k): Dh[s, d] = sum_rows xp[s] xp[s+d] over the first k-1 samples of the zero-padded rows (0 where
    s + d >= k-1), Dt the same over the k-1 samples from position T on (ign_edge_lagprod_fwd; no gradient: input data)."""
    _need_gpu("edge_lagprod", x_rows)
    L = _lib.lib()
    x_rows = x_rows.contiguous()
    R, T = x_rows.shape
    part = torch.empty(int(L.ign_edge_lagprod_parts(R)), 2, 124, 128, device=x_rows.device, dtype=torch.float32)
    _lib.check(L.ign_edge_lagprod_fwd(_ptr(x_rows), _ptr(part), R, T, int(k), int(pad_left), _stream()), "ign_edge_lagprod_fwd")
    tot = part[:, :, :k - 1, :k].sum(dim=0, dtype=torch.float64)
    return tot[0], tot[1]


def conv1_sumsq(x_rows, w1, mu, pad_left):
    return Conv1SumSqFn.apply(x_rows, w1, mu, pad_left)


def bn1_data_stats(x_rows, k, pad_left):
    """(G, S), float64: the window Gram matrix (k, k) and the per-tap sums (k) of the zero-padded rows of `x_rows` (R, T) -- the
    data side of BatchNorm-1's batch statistics (models/eegcnn.py), one C call = four launches (ign_bn1_data_stats: lag sums and
    row sums, edge terms and column sums, float64 sums of the per-block partials, assembly).  No gradient: the operand is input
    data.  2 <= k <= 125, k <= T <= 1024."""
    _need_gpu("bn1_data_stats", x_rows)
    L = _lib.lib()
    x_rows = x_rows.contiguous()
    R, T = x_rows.shape
    dev = x_rows.device
    ws = torch.empty(int(L.ign_bn1_data_stats_workspace_bytes(R, T, int(k))), device=dev, dtype=torch.uint8)
    G = torch.empty(k, k, device=dev, dtype=torch.float64)
    S = torch.empty(k, device=dev, dtype=torch.float64)
    _lib.check(L.ign_bn1_data_stats(_ptr(x_rows), R, T, int(k), int(pad_left), _ptr(ws), _ptr(G), _ptr(S), _stream()),
               "ign_bn1_data_stats")
    return G, S


class Bn1FoldFn(torch.autograd.Function):
    """(w1 (F1,k), gamma, beta (F1), rs (F1*D)) -> (alpha, cshift) (F1*D each): BatchNorm-1 with batch statistics folded into the
    per-channel affine map the fused BatchNorm-2 op absorbs -- mean and variance are the linear / quadratic form of the filter
    over the data statistics (S, G), so forward and backward are closed-form in the parameters (ign_bn1_fold_fwd / _bwd).
    Running statistics (nullable) are updated by the forward launch."""

    @staticmethod
    def forward(ctx, w1, gamma, beta, rs, G, S, n, eps, momentum, run_mean, run_var, Dm):
        _need_gpu("bn1_fold", w1, gamma, beta, rs)
        L = _lib.lib()
        w1, gamma, beta, rs = w1.contiguous(), gamma.contiguous(), beta.contiguous(), rs.contiguous()
        F1, k = w1.shape
        alpha = torch.empty(F1 * Dm, device=w1.device, dtype=torch.float32)
        cshift = torch.empty_like(alpha)
        saved = torch.empty(F1, k + 4, device=w1.device, dtype=torch.float64)
        _lib.check(L.ign_bn1_fold_fwd(_ptr(w1), _ptr(gamma), _ptr(beta), _ptr(rs), _ptr(G), _ptr(S), float(n), float(eps),
                                      float(momentum), _ptr(run_mean), _ptr(run_var), _ptr(alpha), _ptr(cshift), _ptr(saved), F1, k,
                                      int(Dm), _stream()), "ign_bn1_fold_fwd")
        ctx.save_for_backward(w1, gamma, rs, S, saved)
        ctx.meta = (float(n), int(Dm))
        return alpha, cshift

    @staticmethod
    def backward(ctx, g_alpha, g_cshift):
        w1, gamma, rs, S, saved = ctx.saved_tensors
        n, Dm = ctx.meta
        F1, k = w1.shape
        g_alpha, g_cshift = g_alpha.contiguous(), g_cshift.contiguous()
        g_w1 = torch.empty_like(w1)
        g_gamma = torch.empty_like(gamma)
        g_beta = torch.empty_like(gamma)
        g_rs = torch.empty_like(rs)
        _lib.check(_lib.lib().ign_bn1_fold_bwd(_ptr(g_alpha), _ptr(g_cshift), _ptr(w1), _ptr(gamma), _ptr(rs), _ptr(S), _ptr(saved), n,
                                               _ptr(g_w1), _ptr(g_gamma), _ptr(g_beta), _ptr(g_rs), F1, k, Dm, _stream()),
                   "ign_bn1_fold_bwd")
        return g_w1, g_gamma, g_beta, g_rs, None, None, None, None, None, None, None, None


def bn1_fold(w1, gamma, beta, rs, G, S, n, eps, momentum, running_mean, running_var, Dm):
    return Bn1FoldFn.apply(w1, gamma, beta, rs, G, S, n, eps, momentum, running_mean, running_var, Dm)


class DwConv1dFn(torch.autograd.Function):
    """Depthwise 'same' 1-D convolution y[b,c,t] = sum_j w[c,j] xpad[b,c,t+j]  (ign_dwconv1d_*)."""

    @staticmethod
    def forward(ctx, x, w, pad_left):
        _need_gpu("dwconv1d", x, w)
        x, w = x.contiguous(), w.contiguous()
        B, C, T = x.shape
        k = w.shape[1]
        y = torch.empty_like(x)
        _lib.check(_lib.lib().ign_dwconv1d_fwd(_ptr(x), _ptr(w), _ptr(y), B, C, T, k, int(pad_left), 0, _stream()),
                   "ign_dwconv1d_fwd")
        ctx.save_for_backward(x, w)
        ctx.pl = int(pad_left)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        B, C, T = x.shape
        k = w.shape[1]
        gy = gy.contiguous()
        L = _lib.lib()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            _lib.check(L.ign_dwconv1d_fwd(_ptr(gy), _ptr(w), _ptr(gx), B, C, T, k, k - 1 - ctx.pl, 1, _stream()),
                       "ign_dwconv1d_fwd(flip)")
        if ctx.needs_input_grad[1]:
            ws = torch.empty(L.ign_dwconv1d_bwd_weight_workspace_bytes(B, C, k) // 4, device=x.device, dtype=torch.float32)
            gw = torch.empty_like(w)
            _lib.check(L.ign_dwconv1d_bwd_weight(_ptr(x), _ptr(gy), _ptr(gw), _ptr(ws), B, C, T, k, ctx.pl, _stream()),
                       "ign_dwconv1d_bwd_weight")
        return gx, gw, None


def dwconv1d(x, w, pad_left):
    return DwConv1dFn.apply(x, w, pad_left)


class ChanContractFn(torch.autograd.Function):
    """u[b,o,t] = sum_c W[o,c] x[b,c,t]  (ign_chan_contract_*): the EEG-CNN's electrode contraction and pointwise convolution
    (IGN/model/eegcnn.py:71,79) on (B, channels, T) tensors.  Co <= 64, Ci <= 128."""

    @staticmethod
    def _pad64(w_t):                       # (Ci, Co) -> (Ci, 64), zero columns
        return w_t.contiguous() if w_t.shape[1] == 64 else torch.nn.functional.pad(w_t, (0, 64 - w_t.shape[1])).contiguous()

    @staticmethod
    def _run(x, w_oc):
        B, Ci, T = x.shape
        Co = w_oc.shape[0]
        u = torch.empty(B, Co, T, device=x.device, dtype=torch.float32)
        wt = ChanContractFn._pad64(w_oc.t())
        _lib.check(_lib.lib().ign_chan_contract_fwd(_ptr(x), _ptr(wt), _ptr(u), B, Ci, Co, T, _stream()), "ign_chan_contract_fwd")
        return u

    @staticmethod
    def forward(ctx, x, w):
        _need_gpu("chan_contract", x, w)
        if w.shape[0] > 64 or w.shape[1] > 128 or w.shape[1] != x.shape[1]:
            raise _lib.IgnError(f"chan_contract: W {tuple(w.shape)} on x {tuple(x.shape)} (Co <= 64, Ci <= 128)")
        x, w = x.contiguous(), w.contiguous()
        ctx.save_for_backward(x, w)
        return ChanContractFn._run(x, w)

    @staticmethod
    def backward(ctx, gu):
        x, w = ctx.saved_tensors
        gu = gu.contiguous()
        B, Ci, T = x.shape
        Co = w.shape[0]
        L = _lib.lib()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            if Ci > 64:
                raise _lib.IgnError("chan_contract: input gradient needs Ci <= 64 (the electrode axis is data and takes none)")
            gx = ChanContractFn._run(gu, w.t().contiguous())
        if ctx.needs_input_grad[1]:
            ws = torch.empty(L.ign_chan_contract_bwd_weight_workspace_bytes(B, Ci, Co, T) // 4, device=x.device, dtype=torch.float32)
            gw = torch.empty_like(w)
            _lib.check(L.ign_chan_contract_bwd_weight(_ptr(gu), _ptr(x), _ptr(gw), _ptr(ws), B, Ci, Co, T, _stream()),
                       "ign_chan_contract_bwd_weight")
        return gx, gw


def chan_contract(x_bct, w_oc):
    return ChanContractFn.apply(x_bct, w_oc)


class BnEluPoolFn(torch.autograd.Function):
    """AvgPool_P(ELU(BatchNorm_train(alpha * v + c))) for v (B, C, T) -- BatchNorm2d + ELU + AvgPool2d((1,P)) of the EEG-CNN
    block (IGN/model/eegcnn.py:72-74,80-82) as one op over the hand-written kernels, with the per-channel affine map in FRONT
    of the BatchNorm (block 1: BatchNorm-1 folded behind the electrode contraction) absorbed analytically:

        y = alpha v + c;  var_y = alpha^2 var_v;  r = rsqrt(var_y + eps);  z = gamma alpha r (v - mean_v) + beta
        (c cancels in the normalisation: its gradient is exactly 0 -- returned as None; it only enters the running mean)

    backward (dz = ELU'(z) dout / P;  S1 = sum dz,  S2 = sum dz (v - mean_v);  n = B T):
        dgamma = alpha r S2,  dbeta = S1,  dv = gamma alpha r (dz - S1/n - alpha^2 r^2 (v - mean_v) S2 / n),
        dalpha = gamma r^3 eps S2          (the only path: BatchNorm is scale-invariant up to eps)
    The per-channel algebra runs in ign_bn_fold_fwd / _bwd (one launch each, float64), which also applies the running-statistics
    update (momentum, unbiased variance) of nn.BatchNorm2d in place when `run_mean` / `run_var` are given."""

    @staticmethod
    def forward(ctx, v, alpha, cshift, gamma, beta, P, eps, run_mean, run_var, momentum):
        _need_gpu("bn_elu_pool", v, gamma, beta)
        v = v.contiguous()
        B, C, T = v.shape
        L = _lib.lib()
        dev = v.device
        f32 = lambda t: None if t is None else t.detach().float().contiguous()
        alpha32, cshift32, gamma32, beta32 = f32(alpha), f32(cshift), f32(gamma), f32(beta)
        sums = torch.empty(C, 2, device=dev, dtype=torch.float64)
        ws = torch.empty(L.ign_chan_stats_workspace_bytes(B, C) // 8, device=dev, dtype=torch.float64)
        _lib.check(L.ign_chan_stats(_ptr(v), _ptr(sums), _ptr(ws), B, C, T, _stream()), "ign_chan_stats")
        scale32 = torch.empty(C, device=dev, dtype=torch.float32)
        shift32 = torch.empty(C, device=dev, dtype=torch.float32)
        fold = torch.empty(C, 2, device=dev, dtype=torch.float64)            # (mean_v, r)
        _lib.check(L.ign_bn_fold_fwd(_ptr(sums), _ptr(alpha32), _ptr(cshift32), _ptr(gamma32), _ptr(beta32), _ptr(scale32),
                                     _ptr(shift32), _ptr(fold), _ptr(run_mean), _ptr(run_var), C, B * T, float(eps),
                                     float(momentum if momentum is not None else 0.0), _stream()), "ign_bn_fold_fwd")
        out = torch.empty(B, C, T // P, device=dev, dtype=torch.float32)
        _lib.check(L.ign_affine_elu_pool_fwd(_ptr(v), _ptr(scale32), _ptr(shift32), _ptr(out), B, C, T, int(P), _stream()),
                   "ign_affine_elu_pool_fwd")
        ctx.save_for_backward(v, scale32, shift32, fold, alpha32, gamma32)
        ctx.P, ctx.eps = int(P), float(eps)
        return out

    @staticmethod
    def backward(ctx, gout):
        v, scale32, shift32, fold, alpha32, gamma32 = ctx.saved_tensors
        gout = gout.contiguous()
        B, C, T = v.shape
        L = _lib.lib()
        dev = v.device
        mean32 = fold[:, 0].float().contiguous()
        sums = torch.empty(C, 2, device=dev, dtype=torch.float64)
        ws = torch.empty(L.ign_chan_stats_workspace_bytes(B, C) // 8, device=dev, dtype=torch.float64)
        _lib.check(L.ign_bn_elu_pool_bwd_sums(_ptr(v), _ptr(gout), _ptr(scale32), _ptr(shift32), _ptr(mean32), _ptr(sums), _ptr(ws),
                                              B, C, T, ctx.P, _stream()), "ign_bn_elu_pool_bwd_sums")
        coef = torch.empty(6, C, device=dev, dtype=torch.float32)            # ka, kb, kc, dgamma, dbeta, dalpha
        _lib.check(L.ign_bn_fold_bwd(_ptr(sums), _ptr(fold), _ptr(alpha32), _ptr(gamma32), _ptr(coef[0]), _ptr(coef[1]), _ptr(coef[2]),
                                     _ptr(coef[3]), _ptr(coef[4]), _ptr(coef[5]) if alpha32 is not None else None, C, B * T, ctx.eps,
                                     _stream()), "ign_bn_fold_bwd")
        dv = None
        if ctx.needs_input_grad[0]:
            dv = torch.empty_like(v)
            _lib.check(L.ign_bn_elu_pool_bwd_apply(_ptr(v), _ptr(gout), _ptr(scale32), _ptr(shift32), _ptr(coef[0]), _ptr(coef[1]),
                                                   _ptr(coef[2]), _ptr(dv), B, C, T, ctx.P, _stream()), "ign_bn_elu_pool_bwd_apply")
        return dv, (coef[5] if alpha32 is not None else None), None, coef[3], coef[4], None, None, None, None, None


def bn_elu_pool(v, bn, P, alpha=None, cshift=None):
    """BatchNorm2d module `bn` (its weight / bias / running statistics / momentum / eps) + ELU + AvgPool((1,P)) on v (B,C,T);
    `alpha`, `cshift`: per-channel affine map y = alpha v + cshift applied in front of the BatchNorm (see BnEluPoolFn).
    Training mode uses batch statistics and updates the running ones like nn.BatchNorm2d; eval mode uses the running ones."""
    _need_gpu("bn_elu_pool", v)
    C = v.shape[1]
    # affine=False: the identity affine map (constants, no gradient)
    gamma = bn.weight if bn.weight is not None else torch.ones(C, device=v.device, dtype=torch.float32)
    beta = bn.bias if bn.bias is not None else torch.zeros(C, device=v.device, dtype=torch.float32)
    if bn.training or not bn.track_running_stats:
        track = bn.training and bn.track_running_stats
        momentum = bn.momentum
        if track:
            bn.num_batches_tracked.add_(1)
            if momentum is None:      # nn.BatchNorm with momentum=None: cumulative moving average, factor 1 / num_batches_tracked
                momentum = 1.0 / float(bn.num_batches_tracked)
        return BnEluPoolFn.apply(v, alpha, cshift, gamma, beta, P, bn.eps, bn.running_mean if track else None,
                                 bn.running_var if track else None, momentum)
    # eval: z = gamma (alpha v + c - running_mean) / sqrt(running_var + eps) + beta -- an affine map, then the apply kernel
    r = torch.rsqrt(bn.running_var + bn.eps)
    a = alpha if alpha is not None else torch.ones_like(r)
    c = cshift if cshift is not None else torch.zeros_like(r)
    scale = (gamma * a * r).contiguous()
    shift = (gamma * (c - bn.running_mean) * r + beta).contiguous()
    return AffineEluPoolFn.apply(v, scale, shift, P)


class AffineEluPoolFn(torch.autograd.Function):
    """AvgPool_P(ELU(scale[c] v + shift[c])) with gradients to v, scale and shift (the eval-mode form of bn_elu_pool)."""

    @staticmethod
    def forward(ctx, v, scale, shift, P):
        _need_gpu("affine_elu_pool", v, scale, shift)
        v, scale, shift = v.contiguous(), scale.contiguous(), shift.contiguous()
        B, C, T = v.shape
        out = torch.empty(B, C, T // P, device=v.device, dtype=torch.float32)
        _lib.check(_lib.lib().ign_affine_elu_pool_fwd(_ptr(v), _ptr(scale), _ptr(shift), _ptr(out), B, C, T, int(P), _stream()),
                   "ign_affine_elu_pool_fwd")
        ctx.save_for_backward(v, scale, shift)
        ctx.P = int(P)
        return out

    @staticmethod
    def backward(ctx, gout):
        v, scale, shift = ctx.saved_tensors
        gout = gout.contiguous()
        B, C, T = v.shape
        L = _lib.lib()
        zero = torch.zeros_like(scale)
        sums = torch.empty(C, 2, device=v.device, dtype=torch.float64)
        ws = torch.empty(L.ign_chan_stats_workspace_bytes(B, C) // 8, device=v.device, dtype=torch.float64)
        _lib.check(L.ign_bn_elu_pool_bwd_sums(_ptr(v), _ptr(gout), _ptr(scale), _ptr(shift), _ptr(zero), _ptr(sums), _ptr(ws),
                                              B, C, T, ctx.P, _stream()), "ign_bn_elu_pool_bwd_sums")
        dv = None
        if ctx.needs_input_grad[0]:
            dv = torch.empty_like(v)
            _lib.check(L.ign_bn_elu_pool_bwd_apply(_ptr(v), _ptr(gout), _ptr(scale), _ptr(shift), _ptr(scale), _ptr(zero), _ptr(zero),
                                                   _ptr(dv), B, C, T, ctx.P, _stream()), "ign_bn_elu_pool_bwd_apply")
        return dv, sums[:, 1].float(), sums[:, 0].float(), None


class DiversityFn(torch.autograd.Function):
    """mean_{c,i,j} exp(-||w_i - w_j + 1e-6||) (1 - delta_ij) of one shapelet group (IGN/model/Shapelet.py:223-230);
    the kernel produces the loss and its gradient together, backward only scales the saved gradient."""

    @staticmethod
    def forward(ctx, w):
        _need_gpu("diversity", w)
        w = w.contiguous()
        K, C, L = w.shape
        part = torch.empty(C, device=w.device, dtype=torch.float32)
        gw = torch.empty_like(w)
        _lib.check(_lib.lib().ign_diversity_fwd_bwd(_ptr(w), _ptr(part), _ptr(gw), K, C, L, 1e-6, _stream()),
                   "ign_diversity_fwd_bwd")
        ctx.save_for_backward(gw)
        return part.sum()

    @staticmethod
    def backward(ctx, g):
        (gw,) = ctx.saved_tensors
        return gw * g


def diversity(w):
    if not w.is_cuda or w.dtype != torch.float32 or w.shape[0] > 16:
        return None
    return DiversityFn.apply(w)


def _sbm_attn_forward(x, wq, bq, wk, bk, pos, want_lse):
    B, F_ = x.shape
    D = wq.shape[0]
    out = torch.empty(B, F_, device=x.device, dtype=torch.float32)
    lse = torch.empty(B, F_, device=x.device, dtype=torch.float32) if want_lse else None
    _lib.check(_lib.lib().ign_sbm_attn_fwd(_ptr(x), x.stride(0), _ptr(wq), _ptr(bq), _ptr(wk), _ptr(bk), _ptr(pos), _ptr(out),
                                           _ptr(lse), B, F_, D, D ** -0.5, _stream()), "ign_sbm_attn_fwd")
    return out, lse


def _sbm_attn_inputs(x, wq, bq, wk, bk, pos):
    _need_gpu("sbm_attention", x, wq, bq, wk, bk, pos)
    if x.dim() != 2 or x.stride(1) != 1:
        x = x.reshape(x.shape[0], -1).contiguous()
    D = wq.shape[0]
    if wq.numel() != D or wk.shape[0] != D or wk.numel() != D or bq.numel() != D or bk.numel() != D or pos.dim() != 2 \
            or pos.shape[1] != D or pos.shape[0] < x.shape[1]:
        raise _lib.IgnError(f"sbm_attention: shapes x {tuple(x.shape)}, wq {tuple(wq.shape)}, wk {tuple(wk.shape)}, "
                            f"pos {tuple(pos.shape)} do not form a (B,F) x (D,1) x (>=F,D) head")
    return (x,) + tuple(t.contiguous() for t in (wq, bq, wk, bk, pos))


class SbmAttentionFn(torch.autograd.Function):
    """The SBM attention head (models/Shapelet.py SelfAttention) on ign_sbm_attn_fwd / ign_sbm_attn_bwd: the (B,F,F) scores are
    never stored.  Saves x, the parameters, the output and its base-2 log-sum-exp; the backward is four launches that produce
    dx and all five parameter gradients.  No host synchronisation and no state kept across calls: capturable."""

    @staticmethod
    def forward(ctx, x, wq, bq, wk, bk, pos):
        x, wq, bq, wk, bk, pos = _sbm_attn_inputs(x, wq, bq, wk, bk, pos)
        out, lse = _sbm_attn_forward(x, wq, bq, wk, bk, pos, True)
        ctx.save_for_backward(x, wq, bq, wk, bk, pos, out, lse)
        ctx.pos_rows = pos.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        x, wq, bq, wk, bk, pos, out, lse = ctx.saved_tensors
        B, F_ = x.shape
        D = wq.shape[0]
        L = _lib.lib()
        g = g.contiguous()
        gx = torch.empty(B, F_, device=x.device, dtype=torch.float32)
        gwq, gwk = torch.empty_like(wq), torch.empty_like(wk)
        gbq, gbk = torch.empty_like(bq), torch.empty_like(bk)
        gpos = torch.empty_like(pos) if ctx.pos_rows == F_ else torch.zeros_like(pos)   # rows past F get no gradient
        ws = torch.empty(L.ign_sbm_attn_workspace_bytes(B, F_) // 4, device=x.device, dtype=torch.float32)
        _lib.check(L.ign_sbm_attn_bwd(_ptr(x), x.stride(0), _ptr(wq), _ptr(bq), _ptr(wk), _ptr(bk), _ptr(pos), _ptr(out), _ptr(lse),
                                      _ptr(g), _ptr(gx), _ptr(gwq), _ptr(gbq), _ptr(gwk), _ptr(gbk), _ptr(gpos), _ptr(ws), B, F_, D,
                                      D ** -0.5, _stream()), "ign_sbm_attn_bwd")
        need = ctx.needs_input_grad
        return tuple(t if n else None for t, n in zip((gx, gwq, gbq, gwk, gbk, gpos), need))


def sbm_attention(x, wq, bq, wk, bk, pos):
    """o_i = sum_j softmax_j(q_i.k_j / sqrt(D)) x_j with q_i = x_i wq + bq + pos_i, k_j = x_j wk + bk + pos_j, over the F features
    of each row of x (B,F): F.scaled_dot_product_attention(q, k, x[..., None]) of IGN/model/Shapelet.py:126-131 in fp32, also
    inside an autocast region.  x (B,F) fp32 on the GPU; wq / wk (D,1), bq / bk (D), pos (>=F, D) with D = 16.  Without
    autograd (no_grad, eval with frozen inputs) only the forward runs and no log-sum-exp is written."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, wq, bq, wk, bk, pos)):
        return SbmAttentionFn.apply(x, wq, bq, wk, bk, pos)
    return _sbm_attn_forward(*_sbm_attn_inputs(x, wq, bq, wk, bk, pos), False)[0]


def _sbm_bilinear_inputs(u, v, weight):
    _need_gpu("sbm_bilinear", u, v, weight)
    if u.dim() != 2 or tuple(v.shape) != tuple(u.shape) or weight.dim() != 3 or weight.shape[1] != u.shape[1] \
            or weight.shape[2] != u.shape[1]:
        raise _lib.IgnError(f"sbm_bilinear: shapes u {tuple(u.shape)}, v {tuple(v.shape)}, weight {tuple(weight.shape)} do not "
                            f"form a (B,F) x (B,F) x (N,F,F) bilinear head")
    return u.contiguous(), v.contiguous(), weight.contiguous()


def _sbm_bilinear_forward(u, v, w, want_t):
    B, F_ = u.shape
    N = w.shape[0]
    L = _lib.lib()
    out = torch.empty(B, N, device=u.device, dtype=torch.float32)
    t = torch.empty(B, N, F_, device=u.device, dtype=torch.float32) if want_t else None
    ws = torch.empty(L.ign_sbm_bilinear_workspace_bytes(B, F_, N) // 4, device=u.device, dtype=torch.float32)
    _lib.check(L.ign_sbm_bilinear_fwd(_ptr(u), _ptr(v), _ptr(w), _ptr(out), _ptr(t), _ptr(ws), B, F_, N, _stream()),
               "ign_sbm_bilinear_fwd")
    return out, t


class SbmBilinearFn(torch.autograd.Function):
    """The bilinear term of the SBM head (nn.Bilinear without bias, models/Shapelet.py) on ign_sbm_bilinear_fwd / _bwd: three
    fp32 matrix-core GEMMs and no (B,F,F) temporary.  Saves u, v, the weight and, when v needs a gradient, T = (u W_n) (B,N,F);
    the backward computes only the gradients asked for (W frozen: no dW GEMM).  No host synchronisation: capturable."""

    @staticmethod
    def forward(ctx, u, v, weight):
        u, v, weight = _sbm_bilinear_inputs(u, v, weight)
        out, t = _sbm_bilinear_forward(u, v, weight, ctx.needs_input_grad[1])
        ctx.save_for_backward(u, v, weight, t)
        return out

    @staticmethod
    def backward(ctx, g):
        u, v, w, t = ctx.saved_tensors
        B, F_ = u.shape
        N = w.shape[0]
        need_u, need_v, need_w = ctx.needs_input_grad
        g = g.contiguous()
        gu = torch.empty_like(u) if need_u else None
        gv = torch.empty_like(v) if need_v else None
        gw = torch.empty_like(w) if need_w else None
        L = _lib.lib()
        ws = torch.empty(L.ign_sbm_bilinear_workspace_bytes(B, F_, N) // 4, device=u.device, dtype=torch.float32) \
            if need_u and N > 1 else None                     # the per-class partials of gu
        _lib.check(L.ign_sbm_bilinear_bwd(_ptr(u), _ptr(v), _ptr(w), _ptr(t), _ptr(g), _ptr(gu), _ptr(gv), _ptr(gw), _ptr(ws), B, F_,
                                          N, _stream()), "ign_sbm_bilinear_bwd")
        return gu, gv, gw


def sbm_bilinear(u, v, weight):
    """out[b,n] = sum_{i,j} u[b,i] weight[n,i,j] v[b,j]: nn.Bilinear(F, F, N, bias=False)(u, v) of IGN/model/Shapelet.py:199-205
    in exact fp32, also inside an autocast region.  u, v (B,F) and weight (N,F,F) fp32 on the GPU.  Without autograd (no_grad,
    or nothing requires grad) only the forward runs and T is not written."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (u, v, weight)):
        return SbmBilinearFn.apply(u, v, weight)
    return _sbm_bilinear_forward(*_sbm_bilinear_inputs(u, v, weight), False)[0]
