"""Sparse MLM head: vocabulary decoder + cross-entropy on the rows whose
label is not ``ignore_index`` only (csrc/mlm_head.hip).

With MLM labels ~85 % of the token rows are ignored: their logits feed
nothing and their ``dlogits`` rows are zeros that the dense path still
pushes through a dgrad and a wgrad GEMM. This op compacts the live rows
on the device, runs decoder forward, CE forward/backward, dgrad, wgrad and
the bias gradient over those rows, and scatters ``dh`` back (exact zeros
at ignored positions). The live count stays a device int — no host read,
static shapes — so the op sits inside the captured training step.

``RAVNEST_SPARSE_MLM_HEAD=0`` switches it off (the model then returns
dense logits to the criterion as before). When every row is live the op
does the same work as the dense path on the hand GEMMs and is SLOWER than
the library path — see docs/features.md.
"""
from __future__ import annotations

import os

import torch

from ._ext import get_ext

# incremented on every call of the fused path (tests assert on it; inside
# a captured graph only warm-up and capture call into Python)
CALLS = 0


def sparse_mlm_head_enabled() -> bool:
    return os.environ.get("RAVNEST_SPARSE_MLM_HEAD", "1") != "0"


def sparse_mlm_head_supported(weight: torch.Tensor, bias, targets) -> bool:
    """Shapes/dtypes the native op handles (mirrors its TORCH_CHECKs);
    the hidden states are expected in the weight's dtype and device."""
    if bias is None or not torch.is_tensor(targets):
        return False
    hd = weight.shape[1]
    n = targets.numel()
    cap = max((n + 63) // 64 * 64, 128)
    vp = (weight.shape[0] + 127) // 128 * 128
    return (weight.is_cuda and targets.is_cuda
            and weight.dtype == torch.bfloat16
            and bias.dtype == torch.bfloat16
            and targets.dtype == torch.int64
            and hd % 64 == 0 and hd >= 128 and vp >= 128
            and n >= 1
            and cap * vp * 2 < 2 ** 32)


class _SparseMLMHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h2, weight, bias, targets, ignore_index):
        ext = get_ext(required=True)
        (loss_sum, count, logits_c, lse, hc, tc, pos) = ext.mlm_head_fwd(
            h2, weight, bias, targets, ignore_index)
        # intermediates, not inputs/outputs: kept as a plain ctx attribute,
        # so autograd's in-place version checks and saved-tensor hooks do
        # not see them. The backward overwrites logits_c in place (one
        # backward per forward, guarded below) and drops them; a forward
        # whose backward never runs keeps the buffers (logits_c is 4 GB
        # at the BERT-base shape) until its graph node is freed.
        ctx.saved = (logits_c, lse, hc, tc, pos, count)
        ctx.save_for_backward(weight)
        return loss_sum / count.clamp(min=1)

    @staticmethod
    def backward(ctx, dloss):
        if ctx.saved is None:
            raise RuntimeError(
                "sparse_mlm_head_loss: backward ran twice (the saved "
                "logits are consumed in place)")
        logits_c, lse, hc, tc, pos, count = ctx.saved
        ctx.saved = None
        (weight,) = ctx.saved_tensors
        ext = get_ext(required=True)
        dh, dw, db = ext.mlm_head_bwd(dloss, logits_c, lse, hc, tc, pos,
                                      count, weight)
        return dh, dw, db, None, None


def sparse_mlm_head_loss(h: torch.Tensor, weight: torch.Tensor,
                         bias: torch.Tensor, targets: torch.Tensor,
                         ignore_index: int = -100) -> torch.Tensor:
    """Mean CE of ``h @ weight.T + bias`` against ``targets`` over the
    non-ignored rows (0 when there are none). h (..., Hd) bf16 on the GPU,
    targets int64 with one entry per row of h."""
    global CALLS
    CALLS += 1
    h2 = h.reshape(-1, h.shape[-1]).contiguous()
    t2 = targets.reshape(-1).contiguous()
    return _SparseMLMHeadFn.apply(h2, weight.contiguous(),
                                  bias.contiguous(), t2, int(ignore_index))
