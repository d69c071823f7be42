"""Layer-level ops used by the removal networks.

Every function here dispatches to a hand-written HIP kernel (csrc/*.hip) through the C
ABI.  Ops whose kernel is not written yet run through torch-ROCm on the GPU and are
recorded in ``INTERIM`` -- they never fall back to the CPU or to the oracle, and
``RFX_STRICT_NATIVE=1`` turns any interim op into an error (DESIGN.md keeps the
coverage table).
"""
import os

import torch
import torch.nn.functional as F

from . import ops
from .ops import launch, query

INTERIM = set()


def _interim(name):
    if os.environ.get("RFX_STRICT_NATIVE", "0") == "1":
        raise RuntimeError(f"op '{name}' has no HIP kernel yet (RFX_STRICT_NATIVE=1)")
    INTERIM.add(name)


def gelu(x):
    return ops.activation(x, "gelu")


GN_MODES = {"none": 0, "gelu": 1, "glu": 2, "glu_scale_res": 3}


class _GroupNormFn(torch.autograd.Function):
    """GroupNorm fused with GELU / GLU / (res + scale * GLU); backward re-materialises gn(x)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, mode, res, scale, sums=None):
        x16 = x.dtype == torch.bfloat16            # a conv output kept in 16 bits (bf16 mode, ops.bf16_storage)
        if not x16:
            ops._req(x, "x")
        x = x.contiguous()
        gamma, beta = gamma.contiguous(), beta.contiguous()          # read (and their gradients written) as dense vectors
        scale = scale.contiguous() if scale is not None else None
        N, Cc = x.shape[0], x.shape[1]
        S = x.numel() // (N * Cc)
        oshape = list(x.shape)
        if mode >= 2:
            oshape[1] = Cc // 2
        y = torch.empty(oshape, device=x.device, dtype=torch.float32)
        mean = torch.empty(N * groups, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        if sums is not None:
            if not (sums.is_cuda and sums.dtype == torch.float64):
                raise ValueError(f"group_norm: sums are fp64 on the GPU (got {sums.dtype}, {sums.device})")
            sums = sums.contiguous()                   # read as dense (N * groups [, slots], 2)
        given = (sums.shape[1] if sums.dim() == 3 else 1) if sums is not None else 0     # number of partial-sum slots
        if sums is None:
            # the statistics kernel stores one pair per (group, chunk) into its own slot: no zero fill, no atomics
            sums = ops.scratch("rfx_groupnorm_fwd_ws", N, Cc, S, groups, device=x.device, dtype=torch.float64)
            given = -1
        if res is not None:
            ops._req(res, "res")
            res = res.contiguous()
        launch("rfx_groupnorm_fwd_x16" if x16 else "rfx_groupnorm_fwd", x, gamma, beta, N, Cc, S, groups, eps, mode,
               res, scale, sums, given, mean, rstd, y)
        ctx.save_for_backward(x, gamma, beta, mean, rstd, scale)
        ctx.cfg = (N, Cc, S, groups, mode)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, beta, mean, rstd, scale = ctx.saved_tensors
        N, Cc, S, groups, mode = ctx.cfg
        ops._req(gy, "gy")
        gy = gy.contiguous()
        dx = torch.empty_like(x)
        # parameter gradients: straight into the flat gradient buffer when a GradSink is armed and this is the parameter's first
        # gradient of the step (the kernel SETS its outputs); otherwise fresh tensors for autograd's accumulation
        sw = ops.sink_write(gamma, beta, scale if mode == 3 else None, first_write=True)
        if sw is not None:
            dgamma, dbeta, dscale = sw.grads
        else:
            dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
            dscale = torch.empty_like(scale) if mode == 3 else None
        gsum = torch.empty(query("rfx_norm_bwd_work_floats", N, Cc, S, groups), device=x.device, dtype=torch.float32)
        with sw or ops.NO_SINK:
            launch("rfx_groupnorm_bwd_x16" if x.dtype == torch.bfloat16 else "rfx_groupnorm_bwd", x, gamma, beta, mean, rstd, gy,
                   N, Cc, S, groups, mode, scale, gsum, dx, dgamma, dbeta, dscale)
        need = ctx.needs_input_grad                   # one launch forms them all: what was not asked for is dropped here
        dx, dres = dx if need[0] else None, gy if (mode == 3 and need[6]) else None
        if sw is not None:
            return dx, None, None, None, None, None, dres, None, None
        return dx, dgamma if need[1] else None, dbeta if need[2] else None, None, None, None, dres, dscale if need[7] else None, None


def group_norm(x, groups, weight, bias, eps=1e-5, mode="none", res=None, scale=None, sums=None):
    """mode: none | gelu | glu | glu_scale_res (out = res + scale[c] * glu(gn(x))).
    sums: fp64 (N*groups, 2) or (N*groups, slots, 2) {sum, sum^2} already accumulated by the producing GEMM's epilogue."""
    return _GroupNormFn.apply(x, weight, bias, groups, eps, GN_MODES[mode], res, scale, sums)


class _BatchNormFn(torch.autograd.Function):
    """BatchNorm2d (+ReLU).  training=True: batch statistics (and running-stat update by the caller
    from the returned mean / biased var); training=False: running statistics, forward only."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, relu):
        ops._req(x, "x")
        x = x.contiguous()
        gamma, beta = gamma.contiguous(), beta.contiguous()          # read (and their gradients written) as dense vectors
        N, Cc = x.shape[0], x.shape[1]
        S = x.numel() // (N * Cc)
        y = torch.empty_like(x)
        mode = 4 if relu else 0
        if training:
            mean = torch.empty(Cc, device=x.device, dtype=torch.float32)
            rstd = torch.empty_like(mean)
            sums = ops.scratch("rfx_batchnorm_fwd_ws", N, Cc, S, device=x.device, dtype=torch.float64)
            given = 0
        else:
            mean = running_mean.contiguous()
            rstd = torch.rsqrt(running_var + eps)
            sums, given = None, 1
        launch("rfx_batchnorm_fwd", x, gamma, beta, N, Cc, S, eps, mode, given, sums, mean, rstd, y)
        if training and running_mean is not None:
            with torch.no_grad():              # C-length vectors: bookkeeping, nn.BatchNorm2d semantics
                n = N * S
                var = 1.0 / (rstd * rstd) - eps
                running_mean.mul_(1 - momentum).add_(mean, alpha=momentum)
                running_var.mul_(1 - momentum).add_(var * (n / max(n - 1, 1)), alpha=momentum)
        ctx.save_for_backward(x, gamma, beta, mean, rstd)
        ctx.cfg = (N, Cc, S, mode, training)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        N, Cc, S, mode, training = ctx.cfg
        if not training:
            raise ValueError("batch_norm backward in eval mode is not on the reference's path")
        gy = gy.contiguous()
        dx = torch.empty_like(x)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
        work = torch.empty(query("rfx_norm_bwd_work_floats", N, Cc, S, 0), device=x.device, dtype=torch.float32)
        launch("rfx_batchnorm_bwd", x, gamma, beta, mean, rstd, gy, N, Cc, S, mode, work, dx, dgamma, dbeta)
        need = ctx.needs_input_grad                   # one launch forms all three
        return dx if need[0] else None, dgamma if need[1] else None, dbeta if need[2] else None, None, None, None, None, None, None


def batch_norm(x, bn, training, relu=False):
    """bn: nn.BatchNorm2d parameter container (weight, bias, running_mean, running_var)."""
    if training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked += 1
    return _BatchNormFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.momentum,
                              bn.eps, relu)


class _AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kh, kw):
        ops._req(x, "x")
        x = x.contiguous()
        N, Cc, H, W = x.shape
        y = torch.empty((N, Cc, H // kh, W // kw), device=x.device, dtype=torch.float32)
        launch("rfx_avgpool2d_fwd", x, y, N * Cc, H, W, kh, kw)
        ctx.cfg = (N, Cc, H, W, kh, kw)
        return y

    @staticmethod
    def backward(ctx, gy):
        N, Cc, H, W, kh, kw = ctx.cfg
        gx = torch.empty((N, Cc, H, W), device=gy.device, dtype=torch.float32)
        launch("rfx_avgpool2d_bwd", gy.contiguous(), gx, N * Cc, H, W, kh, kw)
        return gx, None, None


def avg_pool2d(x, kernel_size):
    kh, kw = kernel_size
    if (kh, kw) == (1, 1):
        return x
    return _AvgPoolFn.apply(x, kh, kw)


class _GluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ops._req(x, "x")
        x = x.contiguous()
        N, Cc = x.shape[0], x.shape[1]
        if Cc % 2:
            raise ValueError(f"glu: the channel axis halves, got {Cc} channels")
        S = x.numel() // (N * Cc)
        shp = list(x.shape)
        shp[1] = Cc // 2
        y = torch.empty(shp, device=x.device, dtype=torch.float32)
        launch("rfx_glu_fwd", x, y, N, Cc, S)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        N, Cc = x.shape[0], x.shape[1]
        S = x.numel() // (N * Cc)
        gx = torch.empty_like(x)
        launch("rfx_glu_bwd", x, gy.contiguous(), gx, N, Cc, S)
        return gx


def glu(x, dim=1):
    if dim != 1:
        raise ValueError("glu: channel axis (dim=1) only")
    return _GluFn.apply(x)


class _AddFn(torch.autograd.Function):
    """x + alpha * y with y broadcast over any of the 4 dims (N, C, A, B); x contiguous."""

    @staticmethod
    def forward(ctx, x, y, alpha):
        ops._req(x, "x"); ops._req(y, "y")
        if y.dim() != x.dim() or x.dim() not in (3, 4):
            raise ValueError(f"add: x and y of the same rank, 3 or 4 (got {x.dim()} and {y.dim()}): a y of lower rank is not "
                             "broadcast as torch would, give it its singleton axes")
        x = x.contiguous()
        x4 = x if x.dim() == 4 else x.unsqueeze(2)
        y4 = y if y.dim() == 4 else y.unsqueeze(2)
        ye = y4.expand_as(x4)
        out = torch.empty_like(x4)
        N, Cc, A, B = x4.shape
        ys = ye.stride()
        launch("rfx_add_bcast", x4, ye, out, N, Cc, A, B, ys[0], ys[1], ys[2], ys[3], float(alpha))
        ctx.cfg = (tuple(y4.shape), tuple(x4.shape), alpha, y.dim())
        return out if x.dim() == 4 else out.squeeze(2)

    @staticmethod
    def backward(ctx, g):
        yshape, xshape, alpha, ydim = ctx.cfg
        gy = None
        if ctx.needs_input_grad[1]:
            g4 = g if g.dim() == 4 else g.unsqueeze(2)
            if yshape == xshape:
                gy = g4 * alpha if alpha != 1.0 else g4
            elif yshape[0] == 1 and yshape[3] == 1 and yshape[1:3] == xshape[1:3]:
                # reduce over (N, B): (c, a) plays the channel role of rfx_channel_sum
                N, Cc, A, B = xshape
                gy = ops.channel_sum(g4.contiguous().view(N, Cc * A, 1, B)).view(1, Cc, A, 1) * alpha
            else:
                gy = g4.sum_to_size(yshape) * alpha
            if ydim == 3:
                gy = gy.squeeze(2)
        return g if ctx.needs_input_grad[0] else None, gy, None


def add(x, y, alpha=1.0):
    return _AddFn.apply(x, y, alpha)


class _DConvLayerFn(torch.autograd.Function):
    """One depth-layer of the Hybrid Demucs DConv branch, ONE launch per direction (csrc/dconv.hip):
    x + scale * GLU(GN(conv1x1(GELU(GN(conv3_dilated(x)))))) on (N, 48, 256) samples, bf16 arithmetic.
    DCONV_FUSED_BWD (round 4): only the layer INPUT is saved; the backward launch recomputes the forward, returns dL/dx and the
    LayerScale / GroupNorm gradients (per-workgroup partial rows, summed here) and hands dz / a / dh to the two weight-gradient GEMMs.
    Otherwise (round 3 path, bench.py --no-fused-dconv-bwd): the forward also stores h / z (bf16), a and the GroupNorm statistics and
    the backward runs layer by layer on the existing kernels (GroupNorm backward x2, input-gradient GEMM x2, weight-gradient GEMM x2)."""

    @staticmethod
    def forward(ctx, x, w1, b1, g1w, g1b, w2, b2, g2w, g2b, scale, dil, eps, grad_on=True):
        ops._req(x, "x")
        x = x.contiguous()                            # the kernels take dense tensors by pointer, the parameters included
        w1, b1, g1w, g1b, w2, b2, g2w, g2b, scale = (p.contiguous() for p in (w1, b1, g1w, g1b, w2, b2, g2w, g2b, scale))
        N, Cc, T = x.shape
        H = Cc // 4
        out = torch.empty_like(x)
        # grad_on: the CALLER's grad mode (inside Function.forward it is always off, and needs_input_grad ignores no_grad)
        need = grad_on and any(ctx.needs_input_grad)
        fused_bwd = need and DCONV_FUSED_BWD
        h16 = z16 = a_out = stats = None
        if need and not fused_bwd:
            h16 = torch.empty((N, H, T), device=x.device, dtype=torch.bfloat16)
            z16 = torch.empty((N, 2 * Cc, T), device=x.device, dtype=torch.bfloat16)
            a_out = torch.empty((N, H, T), device=x.device, dtype=torch.float32)
            stats = torch.empty((4, N), device=x.device, dtype=torch.float32)
        launch("rfx_dconv_layer_fwd", x, out, N, Cc, T, dil, w1, b1, g1w, g1b, w2, b2, g2w, g2b, scale, float(eps), h16, z16, a_out,
               stats)
        if fused_bwd:
            ctx.save_for_backward(x, w1, b1, g1w, g1b, w2, b2, g2w, g2b, scale)
            ctx.cfg = (dil, float(eps), True)
        elif need:
            ctx.save_for_backward(x, w1, b1, g1w, g1b, w2, b2, g2w, g2b, scale, h16, z16, a_out, stats)
            ctx.cfg = (dil, float(eps), False)
        return out

    @staticmethod
    def backward(ctx, gy):
        dil, eps, fused_bwd = ctx.cfg
        if fused_bwd:
            grads = _DConvLayerFn._backward_fused(ctx, gy, dil, eps)
        else:
            grads = _DConvLayerFn._backward_layers(ctx, gy, dil)
        return tuple(g if n else None for g, n in zip(grads, ctx.needs_input_grad))      # either form computes them all

    @staticmethod
    def _backward_layers(ctx, gy, dil):
        x, w1, b1, g1w, g1b, w2, b2, g2w, g2b, scale, h16, z16, a_out, stats = ctx.saved_tensors
        N, Cc, T = x.shape
        H = Cc // 4
        gy = gy.contiguous()
        # GroupNorm(1, 2C) + GLU + LayerScale backward (mode 3): dz (bf16), dgamma2 / dbeta2 / dscale; the residual passes gy on
        dz = torch.empty_like(z16)
        dg2w, dg2b, dscale = torch.empty_like(g2w), torch.empty_like(g2b), torch.empty_like(scale)
        work = torch.empty(query("rfx_norm_bwd_work_floats", N, 2 * Cc, T, 1), device=x.device, dtype=torch.float32)
        launch("rfx_groupnorm_bwd_x16", z16, g2w, g2b, stats[2], stats[3], gy, N, 2 * Cc, T, 1, 3, scale, work, dz, dg2w, dg2b, dscale)
        # 1x1 convolution: da = W2^T dz;  dW2, db2
        w24 = w2.reshape(2 * Cc, H, 1, 1)
        a4, dz4 = a_out.unsqueeze(2), dz.unsqueeze(2)
        da = ops.conv2d_dgrad(dz4, w24, tuple(a4.shape), tuple(a4.stride()), (1, 1), (0, 0), (1, 1)).squeeze(2)
        dw2, db2 = ops.conv2d_wgrad(a4, dz4, (2 * Cc, H, 1, 1), (1, 1), (0, 0), (1, 1), True, w2, b2)
        # GroupNorm(1, H) + GELU backward (mode 1): dh (bf16), dgamma1 / dbeta1
        dh = torch.empty_like(h16)
        dg1w, dg1b = torch.empty_like(g1w), torch.empty_like(g1b)
        work1 = torch.empty(query("rfx_norm_bwd_work_floats", N, H, T, 1), device=x.device, dtype=torch.float32)
        launch("rfx_groupnorm_bwd_x16", h16, g1w, g1b, stats[0], stats[1], da, N, H, T, 1, 1, None, work1, dh, dg1w, dg1b, None)
        # dilated convolution: dx = W1^T * dh + gy (the residual rides in the GEMM's store);  dW1, db1
        w14 = w1.reshape(H, Cc, 1, 3)
        x4, dh4 = x.unsqueeze(2), dh.unsqueeze(2)
        dx = ops.conv2d_dgrad(dh4, w14, tuple(x4.shape), tuple(x4.stride()), (1, 1), (0, dil), (1, dil), res=gy.unsqueeze(2)).squeeze(2)
        dw1, db1 = ops.conv2d_wgrad(x4, dh4, (H, Cc, 1, 3), (1, 1), (0, dil), (1, dil), True, w1, b1)
        dw2 = dw2.view_as(w2) if dw2 is not None else None           # each convolution takes the sink route (None) or not on its own
        dw1 = dw1.view_as(w1) if dw1 is not None else None
        return dx, dw1, db1, dg1w, dg1b, dw2, db2, dg2w, dg2b, dscale, None, None, None

    @staticmethod
    def _backward_fused(ctx, gy, dil, eps):
        x, w1, b1, g1w, g1b, w2, b2, g2w, g2b, scale = ctx.saved_tensors
        N, Cc, T = x.shape
        H = Cc // 4
        gy = gy.contiguous()
        dx = torch.empty_like(x)
        dz = torch.empty((N, 2 * Cc, T), device=x.device, dtype=torch.bfloat16)
        a_out = torch.empty((N, H, T), device=x.device, dtype=torch.float32)
        dh = torch.empty((N, H, T), device=x.device, dtype=torch.bfloat16)
        partial = ops.scratch("rfx_dconv_layer_bwd_ws", N, Cc, T, dil, device=x.device, dtype=torch.float32)
        launch("rfx_dconv_layer_bwd", x, gy, dx, N, Cc, T, dil, w1, b1, g1w, g1b, w2, b2, g2w, g2b, scale, eps, dz, a_out, dh, partial)
        ps = partial.view(-1, 5 * Cc + 2 * H).sum(0)       # one row per workgroup: dscale | dgn2w | dgn2b | dgn1w | dgn1b
        dscale, dg2w, dg2b = ps[:Cc], ps[Cc:3 * Cc], ps[3 * Cc:5 * Cc]
        dg1w, dg1b = ps[5 * Cc:5 * Cc + H], ps[5 * Cc + H:]
        # weight / bias gradients of the two convolutions on the existing wgrad kernels (side stream + in place when a GradSink is armed)
        dw2, db2 = ops.conv2d_wgrad(a_out.unsqueeze(2), dz.unsqueeze(2), (2 * Cc, H, 1, 1), (1, 1), (0, 0), (1, 1), True, w2, b2)
        dw1, db1 = ops.conv2d_wgrad(x.unsqueeze(2), dh.unsqueeze(2), (H, Cc, 1, 3), (1, 1), (0, dil), (1, dil), True, w1, b1)
        dw2 = dw2.view_as(w2) if dw2 is not None else None
        dw1 = dw1.view_as(w1) if dw1 is not None else None
        return dx, dw1, db1, dg1w, dg1b, dw2, db2, dg2w, dg2b, dscale, None, None, None


# Round 4 measurement (N = 32768 x (48, 256), two depth layers, scripts/perf_dconv.py): fused forward without the h / z / a stores 2.5 ms
# (3.9 with them), but the fused backward launch takes 13.7 ms against 3.0 ms for the four kernels it replaces -- 7 ms of that in the
# LDS float atomics of the parameter-gradient row sums (~100 clocks per ds_add_f32 wave-instruction), the rest in a dependency-bound
# 16-wave lockstep with 424 bytes of scratch per lane.  Correct (tests/test_gpu_dconv_fused.py runs both), not the default.
DCONV_FUSED_BWD = False       # bench.py --fused-dconv-bwd switches the one-launch backward on
DCONV_FUSED = True            # bench.py --no-fused-dconv flips it for A/B runs


def dconv_layer_fused_ok(x, hidden, kernel_size, dil, need_grad):
    """Shapes / mode the fused DConv layer kernel takes (csrc/dconv.hip): bf16 arithmetic, contiguous fp32 (N, 48, 256),
    hidden = 12, kernel 3, dilation 1 or 2."""
    if not DCONV_FUSED or ops.GEMM_PREC != 2 or x.dim() != 3 or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
        return False
    Cc, T = x.shape[1], x.shape[2]
    return hidden * 4 == Cc and kernel_size == 3 and bool(query("rfx_dconv_layer_ok", Cc, T, dil))


def dconv_layer(x, conv1, gn1, conv2, gn2, scale, dil):
    """conv1 / conv2: nn.Conv1d parameter containers, gn1 / gn2: nn.GroupNorm(1, .), scale: the LayerScale vector."""
    return _DConvLayerFn.apply(x, conv1.weight, conv1.bias, gn1.weight, gn1.bias, conv2.weight, conv2.bias, gn2.weight, gn2.bias,
                               scale, int(dil), float(gn1.eps), torch.is_grad_enabled())


class _MulFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ops._req(a, "a"); ops._req(b, "b")
        a, b = a.contiguous(), b.contiguous()
        if a.shape != b.shape:
            raise ValueError("mul: equal shapes")
        y = torch.empty_like(a)
        launch("rfx_mul", a, b, y, a.numel())
        ctx.save_for_backward(a, b)
        return y

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        ga = gb = None
        if ctx.needs_input_grad[0]:
            ga = torch.empty_like(a)
            launch("rfx_mul", g, b, ga, a.numel())
        if ctx.needs_input_grad[1]:
            gb = torch.empty_like(b)
            launch("rfx_mul", g, a, gb, a.numel())
        return ga, gb


def mul(a, b):
    """a * b elementwise (equal shapes) with gradients to both."""
    return _MulFn.apply(a, b)


def row_standardize(x, eps):
    """(x - mean) / (eps + std) over all dims but the first, unbiased std (HDemucs forward); x carries no
    gradient (it is the input waveform / its STFT).  Returns y, mean (R,), std (R,)."""
    x = x.contiguous()
    mean, std, a, b = row_moments(x, eps)
    R = x.shape[0]
    y = torch.empty_like(x)
    launch("rfx_row_affine", x, a, b, y, R, x.numel() // R)
    return y, mean, std


class _RowAffineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, b):
        ops._req(x, "x"); ops._req(a, "a"); ops._req(b, "b")
        x = x.contiguous()
        R = x.shape[0]
        y = torch.empty_like(x)
        launch("rfx_row_affine", x, a, b, y, R, x.numel() // R)
        ctx.save_for_backward(a)
        return y

    @staticmethod
    def backward(ctx, g):
        (a,) = ctx.saved_tensors
        g = g.contiguous()
        R = g.shape[0]
        gx = torch.empty_like(g)
        launch("rfx_row_affine", g, a, None, gx, R, g.numel() // R)
        return gx, None, None


def row_moments(x, eps):
    """Per-row (leading dim) mean, unbiased std and the standardisation coefficients a = 1 / (eps + std), b = -mean a of a tensor that
    carries no gradient -- row_standardize without the affine pass (the consumer applies x a + b itself: clchain.head_conv_fm)."""
    ops._req(x, "x")
    x = x.contiguous()
    R = x.shape[0]
    L = x.numel() // R
    sums = ops.scratch("rfx_row_moments_ws", R, L, device=x.device, dtype=torch.float64)      # one slot per workgroup
    mean = torch.empty(R, device=x.device, dtype=torch.float32)
    std, a, b = torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean)
    launch("rfx_row_moments", x, R, L, sums, mean, std, float(eps), a, b)     # a = 1 / (eps + std), b = -mean a: the finalize kernel
    return mean, std, a, b


def _fm_cm_affine(x, y, a, b, N, group, bins, F, fwd):
    """rfx_fm_cm_affine (one coefficient pair per row) or, for group > 1, rfx_fm_cm_affine_g."""
    if group == 1:
        launch("rfx_fm_cm_affine", x, y, a, b, N, bins, F, fwd)
    else:
        launch("rfx_fm_cm_affine_g", x, y, a, b, N, group, bins, F, fwd)


class _CmToFmAffineFn(torch.autograd.Function):
    """y[n][frame][bin][c] = x[n][c][bin][frame] a[n / group] + b[n / group]: HDemucs' de-standardisation fused with the layout change
    in front of the frame-major inverse STFT; the gradient reaches x only (a, b are detached statistics of the input).  `group`
    consecutive rows share one (a, b) pair: the S * Cin rows of a multi-source HDemucs clip share the clip's statistics."""

    @staticmethod
    def forward(ctx, x, a, b, group):
        ops._req(x, "x")
        x = x.contiguous()
        N, Cc, bins, F = x.shape
        if Cc != 2 or x.dtype != torch.float32 or N % group or (group > 1 and (a.numel() != N // group or b.numel() != N // group)):
            raise ValueError(f"cm_to_fm_affine: (N, 2, bins, frames) fp32 with N / group = {N} / {group} coefficient pairs")
        y = torch.empty((N, F, bins, 2), device=x.device, dtype=torch.float32)
        _fm_cm_affine(x, y, a, b, N, group, bins, F, 1)
        ctx.save_for_backward(a)
        ctx.group = group
        return y

    @staticmethod
    def backward(ctx, g):
        (a,) = ctx.saved_tensors
        g = g.contiguous()
        N, F, bins, _ = g.shape
        gx = torch.empty((N, 2, bins, F), device=g.device, dtype=torch.float32)
        _fm_cm_affine(g, gx, a, None, N, ctx.group, bins, F, 0)
        return gx, None, None, None


def cm_to_fm_affine(x, a, b, group=1):
    """(N, 2, bins, frames) -> (N, frames, bins, 2) times a plus b; `group` consecutive rows share one coefficient pair."""
    return _CmToFmAffineFn.apply(x, a.contiguous(), b.contiguous(), int(group))


def row_affine(x, a, b):
    """x * a[r] + b[r] per leading-dim row (de-standardisation); gradient flows to x only."""
    return _RowAffineFn.apply(x, a.contiguous(), b.contiguous())


class _RowAffineAddFn(torch.autograd.Function):
    """out[r] = x[r] * a[r / group] + b[r / group] + y[r] over rows of equal length (rfx_row_affine_add).  The gradient passes to y
    unchanged and to x through rfx_row_affine with a; a and b are detached statistics."""

    @staticmethod
    def forward(ctx, x, a, b, y, group):
        ops._req(x, "x")
        ops._req(y, "y")
        x, y = x.contiguous(), y.contiguous()
        Q = a.numel()
        R = Q * group
        if x.numel() != y.numel() or x.numel() % R or b.numel() != Q:
            raise ValueError(f"row_affine_add: x {tuple(x.shape)}, y {tuple(y.shape)} against {Q} coefficient pairs for groups of {group} rows")
        out = torch.empty_like(y)
        launch("rfx_row_affine_add", x, a, b, y, out, R, group, x.numel() // R)
        ctx.save_for_backward(a)
        ctx.xshape = x.shape
        return out

    @staticmethod
    def backward(ctx, g):
        (a,) = ctx.saved_tensors
        gx = None
        if ctx.needs_input_grad[0]:
            gc = g.contiguous()
            Q = a.numel()
            gx = torch.empty(ctx.xshape, device=g.device, dtype=torch.float32)
            # the rows of a group are contiguous: one row of group * L samples per coefficient
            launch("rfx_row_affine", gc, a, None, gx, Q, gc.numel() // Q)
        return gx, None, None, g if ctx.needs_input_grad[3] else None, None


def row_affine_add(x, a, b, y, group=1):
    """x * a[r / group] + b[r / group] + y over a.numel() * group rows (every trailing dim flattened); the result takes y's shape.
    Gradients flow to x and y."""
    return _RowAffineAddFn.apply(x, a.contiguous(), b.contiguous(), y, int(group))


class _LocalStateFn(torch.autograd.Function):
    """softmax_t(k^T q / sqrt(ch) + decay penalty, masked diagonal) applied to the content: one HIP launch per direction
    (csrc/attention.hip) instead of two rocBLAS einsums, an ATen softmax and the (B, h, T, T) round trips."""

    @staticmethod
    def forward(ctx, q, k, cont, qd, heads, ndecay):
        for t, n in ((q, "q"), (k, "k"), (cont, "content"), (qd, "query_decay")):
            ops._req(t, n)
        q, k, cont, qd = q.contiguous(), k.contiguous(), cont.contiguous(), qd.contiguous()
        B, Ctot, T = q.shape
        ch = Ctot // heads
        out = torch.empty_like(q)
        need_w = any(ctx.needs_input_grad[:4])
        # bf16 mode: MFMA kernels (attention_mfma.hip), weights recomputed in the backward pass instead of stored
        mfma = ops.GEMM_PREC == 2 and bool(query("rfx_localstate_mfma_ok", B, heads, ch, T, ndecay))
        # more than 256 frames (whole files) or ch * T beyond the LDS-resident kernel: the streaming any-T kernels
        gen = not mfma and (T > 256 or ch * T > 12288 or ndecay > 8)
        if mfma:
            launch("rfx_localstate_mfma_fwd", q, k, cont, qd, B, heads, ch, T, ndecay, out)
            if need_w:
                ctx.save_for_backward(q, k, cont, qd)
        elif gen:
            if ch > 104 or ndecay > 64:
                raise ValueError(f"LocalState attention: {ch} channels per head / {ndecay} decay terms exceed the HIP kernels' "
                                 "limits (ch <= 104, ndecay <= 64)")
            stat = torch.empty((B * heads * T, 4), device=q.device, dtype=torch.float32)
            launch("rfx_localstate_gen_fwd", q, k, cont, qd, B, heads, ch, T, ndecay, stat, out)
            if need_w:
                ctx.save_for_backward(q, k, cont, qd, stat, out)
        else:
            w = torch.empty((B, heads, T, T), device=q.device, dtype=torch.float32) if need_w else None
            launch("rfx_localstate_fwd", q, k, cont, qd, B, heads, ch, T, ndecay, w, out)
            if need_w:
                ctx.save_for_backward(q, k, cont, qd, w)
        ctx.cfg = (B, heads, ch, T, ndecay, mfma, gen)
        return out

    @staticmethod
    def backward(ctx, g):
        B, heads, ch, T, ndecay, mfma, gen = ctx.cfg
        g = g.contiguous()
        q, k, cont, qd = ctx.saved_tensors[:4]
        dq, dk, dc, dqd = torch.empty_like(q), torch.empty_like(k), torch.empty_like(cont), torch.empty_like(qd)
        if mfma:
            stat = torch.empty((B * heads * T, 4), device=q.device, dtype=torch.float32)
            launch("rfx_localstate_mfma_bwd", q, k, cont, qd, g, B, heads, ch, T, ndecay, dq, dk, dc, dqd, stat)
        elif gen:
            stat, out = ctx.saved_tensors[4:6]
            launch("rfx_localstate_gen_bwd", q, k, cont, qd, stat, out, g, B, heads, ch, T, ndecay, dq, dk, dc, dqd)
        else:
            w = ctx.saved_tensors[4]
            launch("rfx_localstate_bwd", q, k, cont, qd, w, g, B, heads, ch, T, ndecay, dq, dk, dc, dqd)
        need = ctx.needs_input_grad                   # one launch forms all four
        return dq if need[0] else None, dk if need[1] else None, dc if need[2] else None, dqd if need[3] else None, None, None


def local_state_attention(q, k, content, query_decay, heads, ndecay):
    """q, k, content: (B, heads*ch, T); query_decay: (B, heads*ndecay, T) raw projections -> (B, heads*ch, T)."""
    return _LocalStateFn.apply(q, k, content, query_decay, heads, ndecay)


class _BlstmFrameFn(torch.autograd.Function):
    """(B, C, T) -> channel-major overlapping frames (1, C, width * B * nfr); rfx_blstm_frames modes 0 / 1."""

    @staticmethod
    def forward(ctx, x, nfr, width, stride):
        ops._req(x, "x")
        x = x.contiguous()
        B, Cc, T = x.shape
        h = torch.empty((1, Cc, width * B * nfr), device=x.device, dtype=torch.float32)
        launch("rfx_blstm_frames", x, None, h, B, Cc, T, nfr, width, stride, 0)
        ctx.cfg = (B, Cc, T, nfr, width, stride)
        return h

    @staticmethod
    def backward(ctx, g):
        B, Cc, T, nfr, width, stride = ctx.cfg
        dx = torch.empty((B, Cc, T), device=g.device, dtype=torch.float32)
        launch("rfx_blstm_frames", g.contiguous(), None, dx, B, Cc, T, nfr, width, stride, 1)
        return dx, None, None, None


class _BlstmUnframeFn(torch.autograd.Function):
    """frames (1, C, width * B * nfr) -> stitched (B, C, T) [+ skip]; rfx_blstm_frames modes 2 / 3."""

    @staticmethod
    def forward(ctx, h, skip, B, T, nfr, width, stride):
        ops._req(h, "h")
        h = h.contiguous()
        Cc = h.shape[1]
        out = torch.empty((B, Cc, T), device=h.device, dtype=torch.float32)
        sk = skip.contiguous() if skip is not None else None
        launch("rfx_blstm_frames", h, sk, out, B, Cc, T, nfr, width, stride, 2)
        ctx.cfg = (B, Cc, T, nfr, width, stride, skip is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        B, Cc, T, nfr, width, stride, has_skip = ctx.cfg
        g = g.contiguous()
        dh = None
        if ctx.needs_input_grad[0]:
            dh = torch.empty((1, Cc, width * B * nfr), device=g.device, dtype=torch.float32)
            launch("rfx_blstm_frames", g, None, dh, B, Cc, T, nfr, width, stride, 3)
        return dh, (g if has_skip and ctx.needs_input_grad[1] else None), None, None, None, None, None


def blstm_frame(x, nfr, width, stride):
    return _BlstmFrameFn.apply(x, nfr, width, stride)


def blstm_unframe(h, skip, B, T, nfr, width, stride):
    return _BlstmUnframeFn.apply(h, skip, B, T, nfr, width, stride)


class _DropoutFn(torch.autograd.Function):
    """F.dropout(x, p, training=True) with a counter-based mask (rfx_dropout): no mask tensor, backward re-draws it."""

    @staticmethod
    def forward(ctx, x, p, seed):
        ops._req(x, "x")
        xc = x.contiguous()
        out = torch.empty_like(xc)
        launch("rfx_dropout", xc, out, xc.numel(), float(p), int(seed))
        ctx.cfg = (float(p), int(seed))
        return out

    @staticmethod
    def backward(ctx, g):
        p, seed = ctx.cfg
        gc = g.contiguous()
        dx = torch.empty_like(gc)
        launch("rfx_dropout", gc, dx, gc.numel(), p, seed)
        return dx, None, None


def dropout(x, p, training=True):
    """The seed is drawn from torch's CPU generator (torch.manual_seed makes runs repeatable; no device sync)."""
    if not training or p <= 0.0:
        return x
    seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    return _DropoutFn.apply(x, float(p), seed)


def linear(x, weight, bias):
    """x: (..., Cin) -> (..., Cout) as a 1x1 gather-GEMM over the flattened rows."""
    shp = x.shape
    x2 = x.reshape(1, -1, shp[-1]).transpose(1, 2)              # (1, Cin, rows) strided view
    y = ops.conv1d(x2, weight.unsqueeze(-1), bias)              # (1, Cout, rows)
    return y.transpose(1, 2).reshape(*shp[:-1], weight.shape[0])
