"""The FCN expert's convolution stack as ONE autograd node over the channels-last implicit-GEMM kernels
(include/ign_abi.h: ign_clconv_*, ign_bn_*; csrc/ign_clconv_{f32,x6}.hip, ign_bn.hip).

Replaces ``block1 -> block2 -> block3 -> AdaptiveAvgPool1d`` of IGN/model/FullyConvNet.py:31-57.  What reaches HBM per
block is only the raw convolution output y_l (needed by the backward anyway): BatchNorm's statistics come out of the
GEMM epilogue, its affine + ReLU are applied while the NEXT GEMM stages its operand, and the last block's
BatchNorm + ReLU + average pool is one reduction pass.  Backward mirrors it: the data-gradient GEMM applies the ReLU
mask of the block below and emits that block's BatchNorm-backward sums; one elementwise pass per block turns them
into dL/dy (written zero-padded, the layout the GEMMs read); the weight-gradient GEMM recomputes relu(bn(y)) on the
fly.  torch supplies memory and the autograd plumbing only.  There is no CPU path.
"""
import ctypes
import os

import torch

from . import _lib, ops


# Arithmetic of the forward / data-gradient GEMMs (the weight gradient is fp32 MFMA in both):
#   "bf16x6": exact 3-way bf16 split of every fp32 operand, six partial products accumulated in fp32 on the bf16 matrix
#             cores -- error vs float64 at the fp32 kernel's level (<= 3e-6 of max; tests/test_gpu_fcn.py), 1.6x its speed;
#   "f32":    v_mfma_f32_32x32x2_f32 (runs at the fp32 VECTOR rate on gfx950);
#   "bf16":   operands rounded to bf16, ONE product, fp32 accumulation -- what torch.autocast(bfloat16) computes for a
#             convolution; selected automatically inside an autocast region (the reference's default mode, `--amp` not passed).
#   "f16x3":  every operand tensor scaled by a power of two (from a device-side bound of its magnitude), split into TWO fp16
#             terms, THREE partial products accumulated in fp32 on the fp16 matrix cores -- the same fp32-level accuracy against
#             float64 as "bf16x6" with half the matrix instructions and two operand planes instead of three (1.5-1.6x its speed;
#             include/ign_abi.h, "h3").  The default in training mode; blocks that normalise with running statistics (eval mode)
#             have no hard bound on their activations and use "bf16x6".
CONV_MATH = os.environ.get("IGN_CONV_MATH", "f16x3")
DEBUG = None       # set to a dict to capture the backward intermediates (tests/diag_fcn.py)


_ptr, _stream = ops._ptr, _lib.stream


def _slot(slots, off):
    """Address of float `off` of the float32 tensor `slots` (the operand bounds of the fp16 path); None without one."""
    return ctypes.c_void_p(slots.data_ptr() + 4 * off) if slots is not None else None


def _fcn_arith(math, autocast, states):
    """The arithmetic (ops.GEMM_*) of the body's GEMMs from fcn_body's `math` argument: the one place that reads CONV_MATH."""
    if math is None:
        math = ops.GEMM_BF16 if autocast else CONV_MATH
    if math == ops.GEMM_H3 and not (all(st.use_batch_stats for st in states) and len(states) <= 8):
        return ops.GEMM_X6          # running statistics: no hard bound on the normalised activations
    return math if math in (ops.GEMM_H3, ops.GEMM_X6, ops.GEMM_BF16) else ops.GEMM_F32


def _wgrad_arith(arith, k):
    """The arithmetic of a block's weight gradient: the split kernels where the tap count is instantiated, else fp32 MFMA."""
    return arith if arith != ops.GEMM_F32 and k in ops.WGRAD_TAPS else ops.GEMM_F32


class BnState:
    """Non-tensor carrier for one block's BatchNorm1d buffers and mode (torch.nn.BatchNorm semantics: batch statistics
    when training or when no running statistics are tracked; the running buffers are updated in place by
    ign_bn_finalize_fwd only in training mode)."""

    def __init__(self, bn):
        self.eps = float(bn.eps)
        self.use_batch_stats = bn.training or not bn.track_running_stats
        self.running_mean = self.running_var = None
        self.momentum = 0.0
        self.bump = None            # the num_batches_tracked counter to increment (fcn_body bumps every block's in ONE launch)
        if bn.track_running_stats:
            self.running_mean, self.running_var = bn.running_mean, bn.running_var
            if bn.training:
                if bn.momentum is None:     # cumulative moving average: the factor needs the counter's value on the host
                    if bn.num_batches_tracked is not None:
                        bn.num_batches_tracked.add_(1)
                    self.momentum = 1.0 / float(bn.num_batches_tracked)
                else:
                    self.bump = bn.num_batches_tracked
                    self.momentum = float(bn.momentum)
        self.update_running = bn.training and bn.track_running_stats


class FcnBodyFn(torch.autograd.Function):
    """forward(x (B,T,C), states, w1, b1, gamma1, beta1, w2, ..., beta3) -> pooled (B, C3).
    The gradient w.r.t. x is opt-in (fcn_body's `input_grad`): without it the backward refuses one, as inputs are data."""

    @staticmethod
    def forward(ctx, x, states_arith, *params):
        L = _lib.lib()
        states, arith, has_head, input_grad, keep = states_arith
        head_w, head_b = (params[-2], params[-1]) if has_head else (None, None)
        if has_head:
            params = params[:-2]
        if not x.is_cuda or x.dtype != torch.float32:
            raise _lib.IgnError(f"fcn_body: needs a float32 GPU tensor, got {x.dtype} on {x.device} (no CPU fallback)")
        x = x.contiguous()
        B = x.shape[0]
        nl = len(params) // 4
        dev = x.device
        f32 = dict(device=dev, dtype=torch.float32)
        need_grad = any(ctx.needs_input_grad[2:2 + len(params)])
        want_gx = bool(input_grad and ctx.needs_input_grad[0])
        # the transposed tap-reversed weights: blocks 2.. whenever a backward runs, block 1 only for the gradient into x
        need_dx = [(need_grad or want_gx) if l else want_gx for l in range(nl)]
        slots = zbuf = xbound = None
        inputs, affine, wds, shapes = [x], [], [], []
        pa = pb = None
        packed = None
        if arith != ops.GEMM_F32 and nl <= 8:
            # prologue: the weights of every block packed (split into bf16 planes) in ONE launch, which also bumps the
            # BatchNorm step counters of the blocks that track running statistics
            ws_ = [params[4 * l].contiguous() for l in range(nl)]
            wts = [torch.empty(int(L.ign_clconv_x3_elems(w.shape[0], w.shape[1], w.shape[2])), device=dev, dtype=torch.bfloat16)
                   for w in ws_]
            wds_ = [torch.empty(int(L.ign_clconv_x3_elems(w.shape[1], w.shape[0], w.shape[2])), device=dev, dtype=torch.bfloat16)
                    if need_dx[l] else None for l, w in enumerate(ws_)]
            vpa, ia, lla = ctypes.c_void_p * nl, ctypes.c_int * nl, ctypes.c_longlong * nl
            pv = lambda ts: vpa(*[(t.data_ptr() if t is not None else None) for t in ts])
            bumps = [st.bump for st in states]
            bump_tab = pv(bumps) if any(b is not None for b in bumps) else None
            dims = (ia(*[w.shape[0] for w in ws_]), ia(*[w.shape[1] for w in ws_]), ia(*[w.shape[2] for w in ws_]))
            if arith == ops.GEMM_H3:
                # operand bounds (4 floats per block: |W|, |block input|, |dL/dy|, spare): weights and the BatchNorm-derived
                # activation bounds from the parameters in one launch, the raw input's from one pass over x
                slots = torch.empty(4 * nl, **f32)
                gam = [None] + [params[4 * (l - 1) + 2].contiguous() for l in range(1, nl)]
                bet = [None] + [params[4 * (l - 1) + 3].contiguous() for l in range(1, nl)]
                Touts, T_ = [], x.shape[1]
                for w in ws_:
                    T_ = T_ - w.shape[2] + 1
                    Touts.append(T_)
                # (the same launch clears the buffer the backward returns as the convolution biases' gradients: a bias in front of
                # a batch-statistics BatchNorm has an identically zero gradient -- the batch mean removes it)
                zbuf = torch.empty(sum(w.shape[0] for w in ws_), **f32) if need_grad else None
                _lib.check(L.ign_fcn_scan(nl, pv(ws_), lla(*[w.numel() for w in ws_]), pv(gam), pv(bet),
                                          ia(*([0] + [ws_[l - 1].shape[0] for l in range(1, nl)])),
                                          lla(*([0] + [B * Touts[l - 1] for l in range(1, nl)])), _ptr(slots), _ptr(zbuf),
                                          zbuf.numel() if zbuf is not None else 0, _stream()), "ign_fcn_scan")
                # max |x|: attached to the tensor by a producer that had the batch in its hands (ops.instance_norm when both
                # experts share a stream), else one pass over x
                xbound = ops.cached_bound(x)
                if xbound is None:
                    _lib.check(L.ign_absmax(_ptr(x), x.numel(), _slot(slots, 1), _stream()), "ign_absmax")
                    xbound = slots[1:2]
                _lib.check(L.ign_clconv_pack_weights_h2_multi(nl, pv(ws_), pv(wts), pv(wds_), *dims, bump_tab,
                                                              vpa(*[slots.data_ptr() + 16 * l for l in range(nl)]), _stream()),
                           "ign_clconv_pack_weights_h2_multi")
            else:
                _lib.check(L.ign_clconv_pack_weights_x3_multi(nl, pv(ws_), pv(wts), pv(wds_), *dims, bump_tab, _stream()),
                           "ign_clconv_pack_weights_x3_multi")
            packed = (wts, wds_)
        else:
            bumps = [st.bump for st in states if st.bump is not None]
            if bumps:
                torch._foreach_add_(bumps, 1)
        for l in range(nl):
            w, b, gamma, beta = (p.contiguous() for p in params[4 * l:4 * l + 4])
            Co, Ci, k = w.shape
            h = inputs[-1]
            Tin = h.shape[1]
            Tout = Tin - k + 1
            if h.shape[2] != Ci or Tout <= 0 or Co % 4:
                raise _lib.IgnError(f"fcn_body block {l + 1}: input {tuple(h.shape)} vs weight {tuple(w.shape)}")
            st = states[l]
            y = torch.empty(B, Tout, Co, **f32)
            nparts = int(L.ign_clconv_mtiles(B * Tout) if arith == ops.GEMM_F32 else L.ign_clconv_x6_mtiles(B, Tout))
            part = torch.empty(nparts, 2, Co, **f32) if st.use_batch_stats else None
            wt, wd = (packed[0][l], packed[1][l]) if packed is not None else ops._pack_weights(arith, w, need_dx[l])
            ops._clconv_fwd(arith, h, wt, b, pa, pb, y, part, (B, Tin, Ci, Co, k), _slot(slots, 4 * l + 1) if l else _ptr(xbound),
                            _slot(slots, 4 * l))
            a, bb, mean, invstd = (torch.empty(Co, **f32) for _ in range(4))
            if st.use_batch_stats:
                _lib.check(L.ign_bn_finalize_fwd(_ptr(part), nparts, B * Tout, Co, _ptr(gamma), _ptr(beta), st.eps, st.momentum,
                                                 _ptr(st.running_mean if st.update_running else None),
                                                 _ptr(st.running_var if st.update_running else None), _ptr(a), _ptr(bb), _ptr(mean),
                                                 _ptr(invstd), _stream()), "ign_bn_finalize_fwd")
            else:
                _lib.check(L.ign_bn_affine_eval(_ptr(st.running_mean), _ptr(st.running_var), _ptr(gamma), _ptr(beta), st.eps, Co,
                                                _ptr(a), _ptr(bb), _ptr(mean), _ptr(invstd), _stream()), "ign_bn_affine_eval")
            inputs.append(y)
            affine.append((a, bb, mean, invstd))
            wds.append(wd)
            shapes.append((Co, Ci, k, Tin, Tout))
            pa, pb = a, bb
        y_last = inputs[-1]
        if keep is not None:
            # opt-in (FullyConvNetwork.keep_last): what the pooling launch below reads, for ops.fcn_cam -- references, no copy
            keep.last_block = (y_last, pa, pb)
        Cl, Tl = y_last.shape[2], y_last.shape[1]
        pooled = torch.empty(B, Cl, **f32)
        head = None
        if has_head:
            # the class head in the pooling launch (a sample's pooled row is complete inside its block)
            head_w = head_w.contiguous()
            N = head_w.shape[0]
            if head_w.shape[1] != Cl or head_w.dtype != torch.float32:
                raise _lib.IgnError(f"fcn_body: head weight {tuple(head_w.shape)} {head_w.dtype} does not fit {Cl} pooled channels")
            out = torch.empty(B, N, **f32)
            _lib.check(L.ign_bn_relu_pool_head_fwd(_ptr(y_last), _ptr(pa), _ptr(pb), _ptr(pooled), _ptr(head_w), _ptr(head_b), _ptr(out),
                                                   B, Tl, Cl, N, _stream()), "ign_bn_relu_pool_head_fwd")
            head = (pooled, head_w, head_b is not None)
        else:
            out = pooled
            _lib.check(L.ign_bn_relu_pool_fwd(_ptr(y_last), _ptr(pa), _ptr(pb), _ptr(pooled), B, Tl, Cl, _stream()),
                       "ign_bn_relu_pool_fwd")
        ctx.head = head
        ctx.head_needs = tuple(ctx.needs_input_grad[-2:]) if has_head else None
        ctx.saved = (inputs, affine, wds, shapes, [st.use_batch_stats for st in states], arith, slots, zbuf, xbound) \
            if (need_grad or want_gx or (has_head and any(ctx.head_needs))) else None
        ctx.body_grad = need_grad
        ctx.want_gx = want_gx
        return out

    @staticmethod
    def backward(ctx, gpool):
        if ctx.saved is None:
            raise _lib.IgnError("fcn_body backward called but the forward ran without parameter gradients enabled")
        if ctx.needs_input_grad[0] and not ctx.want_gx:
            raise _lib.IgnError("fcn_body: gradient w.r.t. the input series is not implemented (inputs are data)")
        L = _lib.lib()
        inputs, affine, wds, shapes, batch_stats, arith, slots, zbuf, xbound = ctx.saved
        nl = len(shapes)
        B = inputs[0].shape[0]
        dev = gpool.device
        f32 = dict(device=dev, dtype=torch.float32)
        gpool = gpool.contiguous()
        need_w, want_gx = ctx.body_grad, ctx.want_gx
        head_grads = ()
        if ctx.head is not None:
            # gpool is the gradient of the LOGITS here: head backward first (pooled-row gradient, weight and bias gradients, one launch;
            # the pooled-row gradient alone in an input-only backward)
            pooled, head_w, has_b = ctx.head
            N, Cl = head_w.shape
            glog = gpool
            gpool = torch.empty(B, Cl, **f32)
            ghw = torch.empty_like(head_w) if (need_w or any(ctx.head_needs)) else None
            ghb = torch.empty(N, **f32) if (has_b and ghw is not None) else None
            _lib.check(L.ign_head_bwd(_ptr(glog), _ptr(pooled), _ptr(head_w), _ptr(gpool), _ptr(ghw), _ptr(ghb), B, Cl, N, Cl, _stream()),
                       "ign_head_bwd")
            head_grads = (ghw if ctx.head_needs[0] else None, ghb if ctx.head_needs[1] else None)
            if not (need_w or want_gx):
                ctx.saved = None
                return (None, None, *([None] * (4 * nl)), *head_grads)
        grads = [None] * (4 * nl)
        # The bias in front of a batch-statistics BatchNorm has an identically zero gradient (the batch mean removes it): the
        # zeros of all blocks are views of ONE buffer (one fill launch)
        zoff, ztot = [], 0
        for (Co_, _, _, _, _), bs_ in zip(shapes, batch_stats):
            zoff.append(ztot)
            ztot += Co_ if bs_ else 0
        if need_w and (zbuf is None or zbuf.numel() != ztot):      # (the fp16 path's forward prologue has cleared one of the right size)
            zbuf = torch.zeros(ztot, **f32) if ztot else None
        # The BatchNorm-backward sums of a block are read by its parameter gradients and, with batch statistics, by dL/dy: an
        # input-only backward (saliency: every parameter frozen) through running statistics needs none of them
        sums = [need_w or bs_ for bs_ in batch_stats]

        # last block: pool -> ReLU mask -> BatchNorm-backward sums
        Co, Ci, k, Tin, Tout = shapes[-1]
        a, bb, mean, invstd = affine[-1]
        y = inputs[-1]
        g = torch.empty_like(y)
        nparts = int(L.ign_bn_relu_pool_bwd_parts(B, Tout))
        part = torch.empty(nparts, 2, Co, **f32) if sums[-1] else None
        _lib.check(L.ign_bn_relu_pool_bwd(_ptr(y), _ptr(gpool), _ptr(a), _ptr(bb), _ptr(mean), _ptr(invstd), _ptr(g), _ptr(part),
                                          B, Tout, Co, _stream()), "ign_bn_relu_pool_bwd")
        # weight-gradient partials of every block are reduced by ONE launch at the end (split-bf16 kernels with k in 2,3,5,8)
        defer = all(_wgrad_arith(arith, sh[2]) != ops.GEMM_F32 for sh in shapes) and nl <= 8
        deferred = []
        gx = None
        for l in range(nl - 1, -1, -1):
            Co, Ci, k, Tin, Tout = shapes[l]
            a, bb, mean, invstd = affine[l]
            y = inputs[l + 1]
            dbeta = dgamma = None
            if sums[l]:
                dbeta, dgamma = torch.empty(Co, **f32), torch.empty(Co, **f32)
                _lib.check(L.ign_bn_finalize_bwd(_ptr(part), nparts, Co, _ptr(dbeta), _ptr(dgamma), _stream()), "ign_bn_finalize_bwd")
            # (the zero rows the data-gradient GEMM reads; the weight gradient skips them: same sums, same bits)
            pad = (k - 1) if (l > 0 or want_gx) else 0
            dyp = torch.empty(B, Tout + 2 * pad, Co, **f32)
            training = 1 if batch_stats[l] else 0
            # (fp16 path: the kernel also takes max |dL/dy| as it writes the tensor -- the bound its two consumers scale by)
            _lib.check(L.ign_bn_bwd_apply_amax(_ptr(g), _ptr(y), _ptr(a), _ptr(mean), _ptr(invstd), _ptr(dbeta), _ptr(dgamma), _ptr(dyp),
                                               _slot(slots, 4 * l + 2), B, Tout, Co, pad, training, _stream()),
                       "ign_bn_bwd_apply_amax")
            if DEBUG is not None:
                DEBUG[f"g{l}"], DEBUG[f"dyp{l}"] = g.clone(), dyp.clone()
                if sums[l]:
                    DEBUG[f"dbeta{l}"], DEBUG[f"dgamma{l}"] = dbeta.clone(), dgamma.clone()
            del g
            if need_w:
                # weight gradient; the operand below is relu(bn(y_{l-1})) recomputed on the fly (raw x for the first block)
                pa, pb = (affine[l - 1][0], affine[l - 1][1]) if l > 0 else (None, None)
                dw = torch.empty(Co, Ci, k, **f32)
                ws = ops._clconv_wgrad(_wgrad_arith(arith, k), dyp, pad, inputs[l], pa, pb, None if defer else dw, (B, Tin, Ci, Co, k),
                                       _slot(slots, 4 * l + 2), _slot(slots, 4 * l + 1) if l else _ptr(xbound))
                if defer:
                    deferred.append((ws, dw, int(L.ign_clconv_wgrad_x6_nsplit(B, Tin, Ci, Co, k)), Co, Ci, k))
                del ws
                grads[4 * l + 0] = dw
                # bias: zero with batch statistics (see above); with running statistics it is the column sum of dL/dy (block 1 padded
                # for the input gradient: summed as the unpadded tensor it otherwise is, so the bits do not depend on that option)
                if training:
                    grads[4 * l + 1] = zbuf[zoff[l]:zoff[l] + Co]
                else:
                    grads[4 * l + 1] = (dyp[:, pad:pad + Tout].contiguous() if (l == 0 and pad) else dyp).sum(dim=(0, 1))
                grads[4 * l + 2] = dgamma
                grads[4 * l + 3] = dbeta
            if l > 0:
                pa_, pb_, pm_, pi_ = affine[l - 1]
                g = torch.empty(B, Tin, Ci, **f32)
                nparts = int(L.ign_clconv_mtiles(B * Tin) if arith == ops.GEMM_F32 else L.ign_clconv_x6_mtiles(B, Tin))
                part = torch.empty(nparts, 2, Ci, **f32) if sums[l - 1] else None
                ops._clconv_dgrad(arith, dyp, wds[l], inputs[l], pa_, pb_, pm_, pi_, g, part, (B, Tin, Ci, Co, k),
                                  _slot(slots, 4 * l + 2), _slot(slots, 4 * l))
            elif want_gx:
                # into the raw series: no block below, plain epilogue, any channel count
                gx = torch.empty(B, Tin, Ci, **f32)
                ops._clconv_dgrad_input(arith, dyp, wds[0], gx, (B, Tin, Ci, Co, k), _slot(slots, 4 * l + 2), _slot(slots, 4 * l))
            del dyp
        if deferred:
            n = len(deferred)
            vpa, ia = ctypes.c_void_p * n, ctypes.c_int * n
            _lib.check(L.ign_clconv_wgrad_reduce_multi(n, vpa(*[d[0].data_ptr() for d in deferred]), vpa(*[d[1].data_ptr() for d in deferred]),
                                                       ia(*[d[2] for d in deferred]), ia(*[d[3] for d in deferred]),
                                                       ia(*[d[4] for d in deferred]), ia(*[d[5] for d in deferred]), _stream()),
                       "ign_clconv_wgrad_reduce_multi")
        ctx.saved = None
        return (gx, None, *grads, *head_grads)


def fcn_body(x, blocks, math=None, head=None, input_grad=False, keep=None):
    """x (B,T,C) float32 on the GPU; blocks = [(conv1d, batchnorm1d), ...] -> pooled (B, C_last).
    `math`: arithmetic of the GEMMs (see CONV_MATH, _fcn_arith); default = "bf16" inside an autocast region, else CONV_MATH.
    `head`: an nn.Linear over the pooled channels (<= ops.HEAD_NMAX outputs) -> its logits (B, N) are returned instead, computed by the
    pooling launch.
    `input_grad`: with it (and x.requires_grad) the backward also returns dL/dx -- block 1's data-gradient GEMM into the raw series
    (ign_clconv_dgrad_input*).  Off (the default) an input that requires a gradient makes the backward raise: inputs are data.  The
    parameter gradients are the same bits either way; with every parameter frozen the backward is input-only (no weight gradient).
    `keep`: an object (the FullyConvNetwork with `keep_last` on) on which this forward leaves `last_block = (y_last, a_last, b_last)`:
    the raw output of the last convolution and that block's BatchNorm affine, as the pooling launch reads them.  None (the default):
    nothing is kept, and no launch or allocation differs."""
    states = [BnState(bn) for _, bn in blocks]            # (the step counters are bumped by the node's prologue launch)
    arith = _fcn_arith(math, torch.is_autocast_enabled(), states)
    params = []
    for conv, bn in blocks:
        if conv.bias is None or bn.weight is None or bn.bias is None:
            raise _lib.IgnError("fcn_body: Conv1d needs a bias and BatchNorm1d needs affine parameters")
        if conv.stride != (1,) or conv.padding != (0,) or conv.dilation != (1,) or conv.groups != 1:
            raise _lib.IgnError("fcn_body: only stride-1, unpadded, undilated, ungrouped Conv1d is implemented")
        params += [conv.weight, conv.bias, bn.weight, bn.bias]
    if head is not None:
        if head.weight.shape[0] > ops.HEAD_NMAX:
            raise _lib.IgnError(f"fcn_body: the fused head covers up to {ops.HEAD_NMAX} outputs")
        # (a head without bias passes a None placeholder: autograd.Function accepts non-tensor inputs)
        return FcnBodyFn.apply(x, (states, arith, True, bool(input_grad), keep), *params, head.weight, head.bias)
    return FcnBodyFn.apply(x, (states, arith, False, bool(input_grad), keep), *params)
