"""Linear projections: library GEMMs by default, hand-written CDNA4 MFMA
GEMM (csrc/gemm.hip — 256^2 glds-staged phase schedule, fused bias/GELU
epilogues) behind RAVNEST_HAND_GEMM=1.

Default path: hipBLASLt (TunableOp-selected algorithms). The hand kernel
measures 0.7-0.8x hipBLASLt on the BERT-base projection shapes
(profiles/r02_gemm_vs_blaslt.txt), so the library stays the default for
the headline bench; the hand path is complete (fwd + dgrad via W^T,
wgrad via library, fused bias-GELU storing the pre-activation) and
numerics-tested, and the flag flips every projection in a model built
through make_linear()/LinearGelu.

NOTE: the transformer models route plain projections through
make_linear() — nn.Linear by default: the explicit backward wins
isolated per-op timings (tools/bench_linear_bwd.py) but loses end-to-end
inside the captured step (see make_linear docstring), so autograd's
addmm backward stays the default. RAVNEST_EXPLICIT_LINEAR=1 flips it.

Weight gradients: make_linear() builds WgradLinear, and LinearGelu and
the bias-downstream projections of BERT call linear() below: forward and
dgrad are the library calls autograd itself makes, dW = dy^T @ x (and the
bias gradient, where routed) come from gemm_wgrad256_bf16 — 256x256
tiles, the reduction split over M, fp32 partials summed in a fixed order
by a finalize kernel that writes bf16 directly (deterministic, no
memset, no cast). RAVNEST_HAND_WGRAD=0 switches it off.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._ext import get_ext


def hand_gemm_enabled() -> bool:
    return os.environ.get("RAVNEST_HAND_GEMM", "0") == "1"


def _hand_ok(x: torch.Tensor, w: torch.Tensor) -> bool:
    """Shapes the hand kernel handles: bf16, K % 64 == 0, K >= 128,
    operands < 4 GiB (32-bit staging offsets)."""
    return (x.is_cuda and x.dtype == torch.bfloat16
            and w.dtype == torch.bfloat16
            and w.shape[1] % 64 == 0 and w.shape[1] >= 128
            and x.numel() * 2 < 2**32 and w.numel() * 2 < 2**32)


def _hand_wgrad_ok(M: int, N: int, K: int) -> bool:
    """Shapes gemm_wgrad_bf16 accepts (M % 64 == 0, M >= 128, N and K
    even and >= 8: its 16-byte staging loads need 4-byte-aligned rows)
    and wins (N*K <= 2304*768)."""
    return (M % 64 == 0 and M >= 128 and N >= 8 and K >= 8
            and N % 2 == 0 and K % 2 == 0 and N * K <= 2304 * 768)


def _hand_wgrad(dy2: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
    """dW = dy^T @ x via the split-K tr16 kernel where it measured
    faster than the library (profiles/r02_gemm_vs_blaslt.txt: wins the
    N*K <= 2304*768 shapes, loses the wide ones)."""
    M, N = dy2.shape
    if _hand_wgrad_ok(M, N, x2.shape[1]):
        ext = get_ext(required=True)
        return ext.gemm_wgrad_bf16(dy2, x2).to(dy2.dtype)
    return dy2.t() @ x2


def _hand_dgrad(dy2: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """dx = dy @ W: reduction over N -> needs W^T as the kernel's
    [rows][k] operand; falls back to the library when N is ragged."""
    N = w.shape[0]
    if N % 64 == 0 and N >= 128 and dy2.numel() * 2 < 2**32:
        ext = get_ext(required=True)
        wt = w.t().contiguous()
        (dx2,) = ext.gemm_nt_bf16(dy2.contiguous(), wt, None, 0)
        return dx2
    return dy2 @ w


class _HandLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ext = get_ext(required=True)
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        if b is not None:
            (y,) = ext.gemm_nt_bf16(x2, w, b.contiguous(), 1)
        else:
            (y,) = ext.gemm_nt_bf16(x2, w, None, 0)
        ctx.save_for_backward(x2, w)
        ctx.has_bias = b is not None
        ctx.x_shape = x.shape
        return y.reshape(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        dx = _hand_dgrad(dy2, w).reshape(ctx.x_shape)
        dw = _hand_wgrad(dy2, x2)
        db = None
        if ctx.has_bias:
            ext = get_ext(required=True)
            db = ext.colsum_bf16(dy2).to(dy.dtype)
        return dx, dw, db


class _HandLinearGeluFn(torch.autograd.Function):
    """y = gelu(x @ W^T + b) in ONE kernel (the epilogue also stores the
    post-bias pre-activation h for the exact backward)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ext = get_ext(required=True)
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        y, h = ext.gemm_nt_bf16(x2, w, b.contiguous(), 2)
        ctx.save_for_backward(x2, w, h)
        ctx.x_shape = x.shape
        return y.reshape(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w, h = ctx.saved_tensors
        ext = get_ext(required=True)
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        # h is POST-bias: reuse the fused gelu-bwd(+colsum) with a zero
        # bias vector
        zb = torch.zeros(w.shape[0], dtype=h.dtype, device=h.device)
        dh, db = ext.bias_gelu_bwd_db(dy2, h, zb)
        dh = dh.contiguous()
        dx = _hand_dgrad(dh, w).reshape(ctx.x_shape)
        dw = dh.t() @ x2
        return dx, dw, db.to(dy.dtype)


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        dx = (dy2 @ w).reshape(x.shape)
        # wgrad GEMM form picked by shape (tools/bench_linear_bwd.py):
        # wide-K projections (mlp_out 3072->768) run 11% faster as
        # mm(x^T, dy)^T (hipBLASLt sees the other TN problem); the rest
        # as the direct dy^T @ x.
        if x2.shape[1] > dy2.shape[1]:
            dw = torch.mm(x2.t(), dy2.contiguous()).t().contiguous()
        else:
            dw = dy2.t() @ x2
        db = None
        if ctx.has_bias:
            ext = get_ext(required=False)
            if dy.is_cuda and dy.dtype == torch.bfloat16 and ext is not None:
                db = ext.colsum_bf16(dy2.contiguous()).to(dy.dtype)
            else:
                db = dy2.sum(0)
        return dx, dw, db


# ---- 256x256 split-M wgrad (csrc/gemm_wgrad.hip, gemm_wgrad256_bf16) ----
def hand_wgrad_enabled() -> bool:
    """RAVNEST_HAND_WGRAD=0 restores autograd's own linear backward (A/B
    inside one build)."""
    return os.environ.get("RAVNEST_HAND_WGRAD", "1") != "0"


def wgrad256_shape_ok(M: int, N: int, K: int) -> bool:
    """Shapes gemm_wgrad256_bf16 accepts: whole 256x256 output tiles and
    whole 64-row reduction tiles, at least two of them."""
    return (N > 0 and K > 0 and N % 256 == 0 and K % 256 == 0
            and M % 64 == 0 and M >= 128)


# (N, K) routed to the kernel, and of those the ones whose bias gradient
# comes from it too. None = every shape the predicate accepts. Filled in
# from the isolated A/B of tools/bench_wgrad.py (profiles/wgrad256.txt).
WGRAD256_ROUTED = None              # all four BERT/GPT-2 shapes won
WGRAD256_DB_ROUTED = {(2304, 768)}  # qkv won; 768x768 (head.dense) lost


def _wgrad256_routed(N: int, K: int) -> bool:
    return WGRAD256_ROUTED is None or (N, K) in WGRAD256_ROUTED


def _wgrad256_db_routed(N: int, K: int) -> bool:
    return WGRAD256_DB_ROUTED is None or (N, K) in WGRAD256_DB_ROUTED


def _wgrad256_applies(x, w) -> bool:
    """Forward-time test: CUDA bf16 tensors of a routed shape, the switch
    on, not under the hand-GEMM flag (which has its own functions)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.bfloat16
            and w.dtype == torch.bfloat16 and x.dim() >= 2
            and hand_wgrad_enabled() and not hand_gemm_enabled()
            and not torch.is_autocast_enabled()):
        return False
    N, K = w.shape
    if x.shape[-1] != K or K == 0:
        return False
    return wgrad256_shape_ok(x.numel() // K, N, K) and _wgrad256_routed(N, K)


def wgrad256(dy2: torch.Tensor, x2: torch.Tensor, want_db: bool):
    """(dW, db or None) of a linear layer from its flattened output
    gradient and input. The kernel takes contiguous operands of an
    accepted shape; anything else runs autograd's own dy^T @ x (and
    dy.sum(0)) — never a copy to make an operand fit."""
    M, N = dy2.shape
    K = x2.shape[1]
    if (dy2.is_cuda and dy2.dtype == torch.bfloat16
            and x2.dtype == torch.bfloat16 and wgrad256_shape_ok(M, N, K)
            and _wgrad256_routed(N, K)
            and dy2.is_contiguous() and x2.is_contiguous()):
        ext = get_ext(required=True)
        if want_db and _wgrad256_db_routed(N, K):
            dw, db = ext.gemm_wgrad256_bf16(dy2, x2, True, False)
            return dw, db
        (dw,) = ext.gemm_wgrad256_bf16(dy2, x2, False, False)
        return dw, (dy2.sum(0) if want_db else None)
    return dy2.t() @ x2, (dy2.sum(0) if want_db else None)


class _Wgrad256LinearFn(torch.autograd.Function):
    """F.linear whose backward takes dW (and db) from gemm_wgrad256_bf16.
    Forward and dgrad are the very library calls autograd's addmm / mm
    path makes (F.linear(x, w, b); dy2 @ w), so their TunableOp
    signatures do not change."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = (dy2 @ w).reshape(x.shape)
        want_db = ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_db:
            dw, db = wgrad256(dy2, x2, want_db)
        return dx, dw, db


def linear(x, w, b=None):
    """F.linear(x, w, b); on CUDA bf16 tensors of a routed shape its
    weight (and bias) gradient comes from the 256x256 wgrad kernel."""
    if _wgrad256_applies(x, w):
        return _Wgrad256LinearFn.apply(x, w, b)
    return F.linear(x, w, b)


class WgradLinear(nn.Linear):
    """nn.Linear (same parameters, same state-dict keys) that runs
    through linear() above. An fx leaf like nn.Linear itself."""
    _is_leaf_module = True

    def forward(self, x):
        return linear(x, self.weight, self.bias)


class Linear(nn.Module):
    """Drop-in nn.Linear replacement (same state-dict keys)."""
    _is_leaf_module = True

    def __init__(self, in_features: int, out_features: int, bias: bool = True):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.zeros(out_features)) if bias else None
        nn.init.normal_(self.weight, std=0.02)

    def forward(self, x):
        if x.is_cuda:
            if hand_gemm_enabled() and _hand_ok(x, self.weight):
                return _HandLinearFn.apply(x, self.weight, self.bias)
            return _LinearFn.apply(x, self.weight, self.bias)
        return F.linear(x, self.weight, self.bias)


def make_linear(in_features: int, out_features: int, bias: bool = True):
    """Projection factory for the model zoo: nn.Linear by default,
    ops.Linear under RAVNEST_EXPLICIT_LINEAR=1 or the hand-GEMM flag
    (same state-dict keys either way).

    Measured both ways twice: the explicit backward wins ISOLATED per-op
    timings on every BERT-base shape (profiles/r02_linear_bwd.txt — qkv
    0.81 vs 0.84 ms, mlp_out 0.81 vs 0.93) but LOSES end-to-end inside
    the captured training step (BERT 1552 vs 1637 samples/s, GPT-2 560
    vs 610 — hipBLASLt/TunableOp pick different algorithms in the graph
    context), so autograd's addmm backward stays the default for dx. (A
    later step profile, profiles/wgrad256.txt section 0, found the same
    GEMM kernels on both paths; the explicit one pays for extra copies,
    fills and column sums.)

    Default: WgradLinear, an nn.Linear whose weight/bias gradient comes
    from the 256x256 split-M wgrad kernel on the shapes it accepts
    (forward and dgrad stay the library calls autograd makes);
    RAVNEST_HAND_WGRAD=0 gives back the plain nn.Linear."""
    if hand_gemm_enabled() or \
            os.environ.get("RAVNEST_EXPLICIT_LINEAR", "0") == "1":
        return Linear(in_features, out_features, bias=bias)
    if hand_wgrad_enabled():
        return WgradLinear(in_features, out_features, bias=bias)
    return nn.Linear(in_features, out_features, bias=bias)
