"""Fused dropout + residual add + LayerNorm: y = LN(a + dropout(z)).

Every BERT layer computes this twice. The composed path (ops/dropout.py
then ops/layernorm.py add_layer_norm) writes the dropped tensor and a byte
mask, reads them back, and in backward reads dy and s three times and
copies the residual gradient. The fused HIP kernels (csrc/dropout_ln.hip)
read z and a once, keep the row in registers, store a 1-bit mask, and
produce dx, dz, dgamma and dbeta from one backward pass.

The mask and the saved sum s are bit-identical to the composed path's for
the same seed: the seed is drawn exactly as ops/dropout.py draws it (one
torch.randint from the CPU generator per call, XORed on the device with the
graph counter of ops/rng.py), so the engine's RNG-replay recompute and the
fresh mask per graph replay are unchanged.

Fused: CUDA bf16 activations, fp32 or bf16 LN parameters, H % 8 == 0 and
H <= 2048, training with p > 0. Everything else takes the composed path.
RAVNEST_FUSED_DROPOUT_LN=0 (read when the module is constructed) selects
the composed path for an A/B inside one build.

zbias: the fused op can also deliver the bias gradient of the Linear that
produced z. dz.sum(0) is what autograd's addmm backward computes for that
bias with a pass of its own over dz, and the backward kernel holds every dz
element in registers just before it stores it. A caller that computed
z = F.linear(x, W, b.detach()) hands b in as zbias: forward ignores it,
backward returns the column sums of dz (fp32 sums of the stored bf16
values, written in b's dtype) as its gradient. Fused path only: asking for
it where the composed path would run is an error, since nothing else would
produce that gradient (DropoutAddLayerNorm.takes_zbias tells beforehand).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from ._ext import get_ext
from .dropout import dropout
from .layernorm import add_layer_norm

_MAX_FUSED_H = 2048  # csrc/dropout_ln.hip keeps the row in registers


class _DropoutAddLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, z, weight, bias, eps, p, zbias):
        ext = get_ext(required=True)
        from . import rng
        # same host draw as _DropoutFn: keeps the CPU generator sequence
        seed = int(torch.randint(0, 2**62, (1,)).item())
        y, s, mean, rstd, maskbits = ext.dropout_add_ln_fwd(
            z, a, weight, bias, eps, p, seed,
            rng.device_seed_counter(a.device))
        ctx.save_for_backward(s, weight, mean, rstd, maskbits)
        ctx.p = p
        ctx.zbias_dtype = None if zbias is None else zbias.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        s, weight, mean, rstd, maskbits = ctx.saved_tensors
        ext = get_ext(required=True)
        # dx and dz are two distinct tensors out of one pass (autograd may
        # steal either for in-place accumulation)
        need = ctx.needs_input_grad
        dzsum = None
        if need[6]:
            dx, dz, dw, db, dzsum = ext.dropout_add_ln_bwd_dzsum(
                dy.contiguous(), s, weight, mean, rstd, maskbits, ctx.p,
                ctx.zbias_dtype == torch.bfloat16)
        else:
            dx, dz, dw, db = ext.dropout_add_ln_bwd(
                dy.contiguous(), s, weight, mean, rstd, maskbits, ctx.p)
        return (dx if need[0] else None, dz if need[1] else None,
                dw if need[2] else None, db if need[3] else None,
                None, None, dzsum)


def _fusable(a, z, weight, bias) -> bool:
    H = a.shape[-1]
    return (a.is_cuda and z.is_cuda
            and a.dtype == torch.bfloat16 and z.dtype == torch.bfloat16
            and a.shape == z.shape
            and H % 8 == 0 and H <= _MAX_FUSED_H
            and weight.dtype == bias.dtype
            and weight.dtype in (torch.float32, torch.bfloat16))


def _zbias_ok(zbias, H) -> bool:
    return (zbias.is_cuda and zbias.shape == (H,)
            and zbias.dtype in (torch.float32, torch.bfloat16))


def dropout_add_layer_norm(a, z, weight, bias, eps: float = 1e-12,
                           p: float = 0.1, training: bool = True,
                           fused: bool = True, zbias=None):
    """y = LayerNorm(a + dropout(z, p)); a is the residual input. zbias:
    see the module docstring."""
    if fused and training and 0.0 < p < 1.0 and _fusable(a, z, weight, bias):
        if zbias is None or _zbias_ok(zbias, a.shape[-1]):
            return _DropoutAddLayerNormFn.apply(
                a.contiguous(), z.contiguous(), weight, bias, eps, p, zbias)
    if zbias is not None:
        raise RuntimeError(
            "dropout_add_layer_norm: zbias needs the fused path (training, "
            "0 < p < 1, CUDA bf16 activations, a fp32 or bf16 bias of the "
            "hidden size)")
    return add_layer_norm(a, dropout(z, p, training), weight, bias, eps)


class DropoutAddLayerNorm(nn.Module):
    """forward(a, z) = LayerNorm(a + dropout(z)); parameters are named as
    AddLayerNorm's, so state-dict keys do not depend on which is used."""
    _is_leaf_module = True

    def __init__(self, hidden: int, eps: float = 1e-12, p: float = 0.1):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden))
        self.bias = nn.Parameter(torch.zeros(hidden))
        self.eps = eps
        self.p = p
        self.fused = os.environ.get("RAVNEST_FUSED_DROPOUT_LN", "1") != "0"

    def takes_zbias(self, a, lin) -> bool:
        """True when forward(a, z, zbias=lin.bias) will take the fused
        path for z = F.linear(x, lin.weight, lin.bias.detach()) of a's
        shape and dtype, so lin's bias gradient can come out of this
        op's backward."""
        b = lin.bias
        return (self.fused and self.training and 0.0 < self.p < 1.0
                and torch.is_tensor(a) and b is not None
                and lin.weight.dtype == a.dtype
                and lin.weight.shape[0] == a.shape[-1]
                and not torch.is_autocast_enabled()
                and _fusable(a, a, self.weight, self.bias)
                and _zbias_ok(b, a.shape[-1]))

    def forward(self, a, z, zbias=None):
        return dropout_add_layer_norm(a, z, self.weight, self.bias, self.eps,
                                      self.p, self.training, self.fused,
                                      zbias)
