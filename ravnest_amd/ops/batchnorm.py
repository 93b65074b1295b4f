"""Fused BatchNorm2d (NCHW) on CDNA4.

Reference workload parity: BatchNorm in CNN/ResNet/Inception (SURVEY.md
section 2.3 standalone BN fwd/bwd row). GPU path: csrc/batchnorm.hip
(per-channel block reductions, fp32 statistics from one read of x as sums
shifted by the channel's first element, not Welford); CPU path: torch
native. In eval mode the backward is dx = dy * w * rstd (frozen-BN
fine-tuning). Drop-in state-dict compatible with nn.BatchNorm2d.

FusedBatchNormReLU2d and FusedBatchNormAddReLU2d fold the ReLU, and the
residual add in front of it, into the apply kernels of both directions:
y = relu(bn(x)) and y = relu(bn(x) + residual). The statistics kernel is
FusedBatchNorm2d's own and the backward reads the ReLU mask from the saved
output, so every result equals the composed path's (BN kernel, torch add,
torch ReLU) bit for bit. RAVNEST_FUSED_BN_RELU=0 (read when the module is
constructed) selects the composed path for an A/B inside one build.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._ext import get_ext


class _BatchNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, running_mean, running_var, training, momentum,
                eps):
        ext = get_ext(required=True)
        y, mean, rstd = ext.batchnorm_fwd(x, w.float(), b.float(),
                                          running_mean, running_var,
                                          training, momentum, eps)
        ctx.save_for_backward(x, w, mean, rstd)
        ctx.training = training
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mean, rstd = ctx.saved_tensors
        ext = get_ext(required=True)
        dx, dw, db = ext.batchnorm_bwd(dy.contiguous(), x, w.float(), mean,
                                       rstd, ctx.training)
        return dx, dw.to(w.dtype), db.to(w.dtype), None, None, None, None, \
            None


class FusedBatchNorm2d(nn.Module):
    _is_leaf_module = True

    def __init__(self, num_features: int, eps: float = 1e-5,
                 momentum: float = 0.1):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.momentum = momentum
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked",
                             torch.tensor(0, dtype=torch.long))

    def forward(self, x):
        if x.is_cuda:
            # stat buffers stay fp32 even under model.to(bf16): the kernel
            # updates them in place at fp32 precision
            if self.running_mean.dtype != torch.float32:
                self.running_mean.data = self.running_mean.data.float()
                self.running_var.data = self.running_var.data.float()
            if self.training:
                self.num_batches_tracked += 1
            return _BatchNormFn.apply(x.contiguous(), self.weight, self.bias,
                                      self.running_mean, self.running_var,
                                      self.training, self.momentum, self.eps)
        return F.batch_norm(x, self.running_mean, self.running_var,
                            self.weight, self.bias, self.training,
                            self.momentum, self.eps)


class _BatchNormReLUFn(torch.autograd.Function):
    """relu(bn(x)) or, with a residual, relu(bn(x) + residual)."""

    @staticmethod
    def forward(ctx, x, residual, w, b, running_mean, running_var, training,
                momentum, eps):
        ext = get_ext(required=True)
        y, mean, rstd = ext.batchnorm_relu_fwd(x, residual, w.float(),
                                               b.float(), running_mean,
                                               running_var, training,
                                               momentum, eps)
        # the ReLU mask is read back from y, as threshold_backward does
        ctx.save_for_backward(x, y, w, mean, rstd)
        ctx.training = training
        ctx.has_residual = residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, w, mean, rstd = ctx.saved_tensors
        ext = get_ext(required=True)
        need = ctx.needs_input_grad
        want_dr = ctx.has_residual and need[1]
        # dx and the residual's gradient are two distinct tensors out of one
        # pass (autograd may steal either for in-place accumulation)
        out = ext.batchnorm_relu_bwd(dy.contiguous(), x, y, w.float(), mean,
                                     rstd, ctx.training, want_dr)
        dx, dw, db = out[:3]
        return (dx if need[0] else None, out[3] if want_dr else None,
                dw.to(w.dtype) if need[2] else None,
                db.to(w.dtype) if need[3] else None,
                None, None, None, None, None)


def bn_relu_launch_constants():
    """(grid cap, block size, bytes per lane) of the two BN+ReLU elementwise
    kernels: one grid-stride trip covers cap * block * bytes / element size
    elements."""
    return tuple(get_ext(required=True).batchnorm_relu_launch_constants())


class _BatchNormActBase(FusedBatchNorm2d):
    def __init__(self, num_features: int, eps: float = 1e-5,
                 momentum: float = 0.1):
        super().__init__(num_features, eps, momentum)
        self.fused = os.environ.get("RAVNEST_FUSED_BN_RELU", "1") != "0"

    def _bn_act(self, x, residual):
        if x.is_cuda and self.fused:
            if self.running_mean.dtype != torch.float32:
                self.running_mean.data = self.running_mean.data.float()
                self.running_var.data = self.running_var.data.float()
            if self.training:
                self.num_batches_tracked += 1
            if residual is not None:
                residual = residual.contiguous()
            return _BatchNormReLUFn.apply(
                x.contiguous(), residual, self.weight, self.bias,
                self.running_mean, self.running_var, self.training,
                self.momentum, self.eps)
        # CPU, or the composed path on the GPU: BN, then add, then ReLU
        y = FusedBatchNorm2d.forward(self, x)
        if residual is not None:
            y = y + residual
        return F.relu(y)


class FusedBatchNormReLU2d(_BatchNormActBase):
    """forward(x) = relu(bn(x)); parameters and buffers are named as
    FusedBatchNorm2d's, so state-dict keys do not depend on which is used."""

    def forward(self, x):
        return self._bn_act(x, None)


class FusedBatchNormAddReLU2d(_BatchNormActBase):
    """forward(x, residual) = relu(bn(x) + residual): a residual block's
    tail. State-dict keys are FusedBatchNorm2d's."""

    def forward(self, x, residual):
        return self._bn_act(x, residual)
