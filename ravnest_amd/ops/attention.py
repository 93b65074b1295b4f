"""Fused multi-head attention core (flash-style forward on CDNA4).

Reference workload parity: minGPT causal self-attention
(model_without_padding_mask.py:50-113) and BERT's padded-mask attention —
SURVEY.md section 2.3. Forward is the hand-written HIP kernel: per Q-tile
online-softmax over K/V tiles, bf16 MFMA (32x32x16), XOR-swizzled LDS
tiles, no S x S score matrix in HBM; it returns O and the log-sum-exp
rows. At D=64 without probability dropout that is csrc/attention_fwd64.hip
(64-key stages, K and V both staged by LDS-DMA, one running-max decision
per stage). FWD64 off (RAVNEST_ATTN_FWD64=0) keeps the 32-key-tile kernel
of csrc/attention.hip, which probability dropout and D=128 always use; it
is the A/B arm of tools/attn_bench.py. Backward runs the fused flash
backward kernels (P recomputed from (Q,K,lse) on-chip), separate and
packed layouts alike. At D=64 that is csrc/attention_bwd64.hip: delta,
one kernel for dK and dV, one for dQ, both on 64-row stages (7 matmul
passes, 3 launches). BWD64 off (RAVNEST_ATTN_BWD64=0) keeps the earlier
delta + dv + dk + dq kernels on 32-row tiles of csrc/attention_bwd.hip
(8 passes, 4 launches), which fused probability dropout always uses; it
is the A/B arm of tools/attn_bench.py. At D=128 it is
csrc/attention_bwd128.hip (delta + dv + dk + dq). BWD_D128 off
(RAVNEST_ATTN_BWD_D128=0) sends D=128 back to the composed backward that
recomputes P with hipBLASLt GEMMs + elementwise torch and materialises
(B,H,S,S) tensors; it is kept as the A/B arm of tools/attn_bench.py.
Cached decoding, one new query per head against a key/value cache, is
csrc/attention_decode.hip (attention_decode below): split-KV, fp32
vector math, no MFMA, no backward.

Shapes: q,k,v (B, H, S, D); additive mask broadcastable to (B, 1, S, S)
or None; causal flag for GPT-style models.

Padded batches: kv_len, an integer (B,) tensor of per-sequence key
counts, bounds the keys of sequence b to [0, kv_len[b]) (clamped to
[1, S]). The kernels read it on the device and never visit key tiles past
it, so attention over a right-padded batch costs what its real tokens
cost. With KV_SKIP on (RAVNEST_ATTN_KV_SKIP=1) a (B,1,1,S) additive
padding mask yields that bound by itself: one small kernel per attention
call finds the last key above -10000 per row, and skipping the dead tail
changes no output bit (a key at -10000 already contributes
exp(-10000 + s - m) == 0). It is off by default: on the all-ones masks of
the BERT benchmark the twelve extra launches per step buy nothing and
measured -0.6 % (profiles/attn_kv_len.txt); turn it on for padded data.
Not for masks whose entries <= -10000 are meant to keep a weight.

Unpadded batches: attention_varlen_qkv runs attention within each
sequence of a packed (T,3,H,D) token stream given by cu_seqlens, so padded
query rows cost nothing either (csrc/attention_varlen64.hip: bf16, D=64,
no mask, kv_len or probability dropout; grids from shapes only, a device
tile table from varlen_tiles). unpad_batch packs a padded (B,S) batch.
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn as nn

from ._ext import get_ext


# Derive the key horizon from the padding mask (module docstring). Read at
# call time: flip ravnest_amd.ops.attention.KV_SKIP to compare both paths.
KV_SKIP = os.environ.get("RAVNEST_ATTN_KV_SKIP", "0") == "1"

# D=128 backward through the flash kernels (and the packed layout through
# _AttnQKVFn). Read at call time; off = the composed backward.
BWD_D128 = os.environ.get("RAVNEST_ATTN_BWD_D128", "1") != "0"

# D=64 backward on 64-row stages with the merged dK/dV kernel. Read at
# call time; off = the 32-row dv, dk and dq kernels.
BWD64 = os.environ.get("RAVNEST_ATTN_BWD64", "1") != "0"

# D=64 forward on 64-key stages (no probability dropout). Read at call
# time; off = the 32-key-tile kernel.
FWD64 = os.environ.get("RAVNEST_ATTN_FWD64", "1") != "0"


def kv_len_from_mask(mask):
    """Additive padding mask, one value per (batch, key) -- (B,S) or
    (B,1,1,S) -- to int32 (B,): 1 + the last key whose entry is above
    -10000, or S for a row without one. Torch twin of the
    attn_mask_kv_len kernel."""
    B, S = mask.shape[0], mask.shape[-1]
    live = mask.reshape(B, S).float() > -10000.0
    pos = torch.arange(1, S + 1, device=mask.device)
    last = (live * pos).amax(dim=1)
    return torch.where(last > 0, last, S).to(torch.int32)


def _per_key_mask(mask, B, S):
    return (mask is not None and mask.shape[0] == B and mask.shape[-1] == S
            and mask.numel() == B * S)


def _as_kv_len(kv_len, B, device):
    if kv_len is None:
        return None
    if kv_len.shape != (B,) or kv_len.is_floating_point():
        raise ValueError(f"kv_len must be an integer tensor of shape ({B},)")
    return kv_len.to(device=device, dtype=torch.int32).contiguous()


def _kv_len_mask(kv_len, S):
    """(B,1,1,S) additive mask with -inf on columns >= kv_len[b] (clamped
    to [1, S] like the kernels do): the composed paths' form of kv_len."""
    cols = torch.arange(S, device=kv_len.device)
    dead = cols[None, :] >= kv_len.clamp(1, S)[:, None]
    m = torch.zeros(dead.shape, device=kv_len.device)
    return m.masked_fill_(dead, float("-inf"))[:, None, None, :]


def _math_attention(q, k, v, mask, causal, scale, kv_len=None):
    s = (q @ k.transpose(-2, -1)) * scale
    if kv_len is not None:
        s = s + _kv_len_mask(kv_len, k.shape[-2])
    if causal:
        S = q.shape[-2]
        cm = torch.full((S, S), float("-inf"), device=q.device)
        cm = torch.triu(cm, diagonal=1)
        s = s + cm
    if mask is not None:
        s = s + mask
    p = torch.softmax(s.float(), dim=-1).to(q.dtype)
    return p @ v


class _AttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, mask, causal, scale, kv_len=None):
        ext = get_ext(required=True)
        if (kv_len is None and KV_SKIP
                and _per_key_mask(mask, q.shape[0], q.shape[2])):
            kv_len = ext.attn_mask_kv_len(mask)
        o, lse = ext.attn_fwd(q, k, v,
                              mask if mask is not None else torch.Tensor(),
                              causal, scale, kv_len, FWD64)
        ctx.save_for_backward(q, k, v, mask if mask is not None else None,
                              o, lse, kv_len)
        ctx.causal = causal
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, mask, o, lse, kv_len = ctx.saved_tensors
        causal, scale = ctx.causal, ctx.scale
        do = do.contiguous()
        D = q.shape[-1]
        if D == 64 or (D == 128 and BWD_D128):
            ext = get_ext(required=True)
            dq, dk, dv = ext.attn_bwd(
                q, k, v, o, do, lse,
                mask if mask is not None else torch.Tensor(), causal, scale,
                kv_len, BWD64)
            return dq, dk, dv, None, None, None, None
        # composed arm (D=128 with BWD_D128 off): recompute P from lse via
        # library GEMMs
        # P = exp(S*scale + mask - lse)
        s = (q @ k.transpose(-2, -1)).float() * scale
        if causal:
            S = q.shape[-2]
            cm = torch.triu(torch.full((S, S), float("-inf"),
                                       device=q.device), diagonal=1)
            s = s + cm
        if mask is not None:
            s = s + mask.float()
        if kv_len is not None:
            s = s + _kv_len_mask(kv_len, k.shape[-2])
        p = torch.exp(s - lse.unsqueeze(-1)).to(q.dtype)
        dv = p.transpose(-2, -1) @ do
        dp = (do @ v.transpose(-2, -1)).float()
        delta = (do.float() * o.float()).sum(-1, keepdim=True)
        ds = (p.float() * (dp - delta)) * scale
        ds = ds.to(q.dtype)
        dq = ds @ k
        dk = ds.transpose(-2, -1) @ q
        return dq, dk, dv, None, None, None, None


def attention(q, k, v, mask=None, causal=False, scale=None, kv_len=None):
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    kv_len = _as_kv_len(kv_len, q.shape[0], q.device)
    if q.is_cuda:
        return _AttnFn.apply(q.contiguous(), k.contiguous(), v.contiguous(),
                             mask, causal, scale, kv_len)
    return _math_attention(q, k, v, mask, causal, scale, kv_len)


class AttentionCore(nn.Module):
    _is_leaf_module = True

    def __init__(self, causal: bool = False):
        super().__init__()
        self.causal = causal

    def forward(self, q, k, v, mask=None, kv_len=None):
        return attention(q, k, v, mask=mask, causal=self.causal,
                         kv_len=kv_len)


class _AttnQKVFn(torch.autograd.Function):
    """Packed path: qkv (B,S,3,H,D) -> o (B,S,H,D). No permute/contiguous
    copies: the kernel reads the projection's natural layout and writes O
    in token-major order (the next Linear's input layout).

    pdrop > 0 fuses attention-PROB dropout (HF BertSelfAttention
    semantics) into the fwd and bwd kernels: the philox seed is drawn
    from the torch CPU generator (so the versioned-recompute engine's
    fork_rng replay redraws the identical mask) and XORed with the
    device graph counter at run time (fresh masks per hipGraph replay).
    The fwd publishes its keep-mask as one 32-key word per (bh, qrow)
    k-block; the three bwd kernels READ those words (regenerating via
    philox measured ~4x the masking cost)."""

    @staticmethod
    def forward(ctx, qkv, mask, causal, scale, pdrop=0.0, kv_len=None):
        ext = get_ext(required=True)
        if (kv_len is None and KV_SKIP
                and _per_key_mask(mask, qkv.shape[0], qkv.shape[1])):
            kv_len = ext.attn_mask_kv_len(mask)
        seed = 0
        seed_buf = None
        if pdrop > 0:
            from . import rng
            seed = int(torch.randint(0, 2**62, (1,)).item())
            seed_buf = rng.device_seed_counter(qkv.device)
        res = ext.attn_fwd_qkv(qkv,
                               mask if mask is not None else torch.Tensor(),
                               causal, scale, pdrop, seed, seed_buf, kv_len,
                               FWD64)
        o, lse = res[0], res[1]
        mbits = res[2] if len(res) > 2 else None
        ctx.save_for_backward(qkv, mask if mask is not None else None, o,
                              lse, mbits, kv_len)
        ctx.causal = causal
        ctx.scale = scale
        ctx.pdrop = pdrop
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, mask, o, lse, mbits, kv_len = ctx.saved_tensors
        ext = get_ext(required=True)
        dqkv = ext.attn_bwd_qkv(
            qkv, o, do.contiguous(), lse,
            mask if mask is not None else torch.Tensor(),
            ctx.causal, ctx.scale, ctx.pdrop, mbits, kv_len, BWD64)
        return dqkv, None, None, None, None, None


def attention_qkv(qkv, mask=None, causal=False, scale=None,
                  prob_dropout=0.0, kv_len=None):
    """qkv (B,S,3,H,D) -> (B,S,H*D). prob_dropout fuses attention-prob
    dropout into the kernels (D=64 path). D=128 takes the packed kernels
    too unless prob_dropout > 0 or BWD_D128 is off. kv_len: see the
    module docstring."""
    H, D = qkv.shape[-2], qkv.shape[-1]
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    kv_len = _as_kv_len(kv_len, qkv.shape[0], qkv.device)
    if qkv.is_cuda and (D == 64 or (D == 128 and BWD_D128
                                    and prob_dropout == 0)):
        o = _AttnQKVFn.apply(qkv.contiguous(), mask, causal, scale,
                             prob_dropout, kv_len)
        return o.flatten(2)
    # fallback: unpack + (custom or math) attention
    q, k, v = (qkv.permute(2, 0, 3, 1, 4)[i] for i in range(3))
    o = attention(q.contiguous(), k.contiguous(), v.contiguous(),
                  mask=mask, causal=causal, scale=scale, kv_len=kv_len)
    return o.transpose(1, 2).flatten(2)


def attention_qkv_prob_dropout(qkv, mask, causal, scale, p, training,
                               kv_len=None):
    """Attention with dropout ON THE PROBABILITIES — exact HuggingFace
    BertSelfAttention semantics. Composed path: the S x S probs are
    materialized and masked by the replayable philox dropout kernel
    (csrc/dropout.hip), so the versioned-recompute engine replays the
    identical mask. Slower than the fused flash kernel (which cannot
    drop individual probs without a P-materialization); use when exact
    prob-dropout semantics matter more than throughput."""
    from .dropout import dropout as _phil_dropout
    q, k, v = qkv.unbind(dim=2)          # (B, S, H, D) each
    q = q.transpose(1, 2)                # (B, H, S, D)
    k = k.transpose(1, 2)
    v = v.transpose(1, 2)
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    s = (q @ k.transpose(-2, -1)) * scale
    if causal:
        S = q.shape[-2]
        cm = torch.triu(torch.full((S, S), float("-inf"),
                                   device=q.device), diagonal=1)
        s = s + cm
    if mask is not None:
        s = s + mask
    kv_len = _as_kv_len(kv_len, qkv.shape[0], qkv.device)
    if kv_len is not None:
        s = s + _kv_len_mask(kv_len, k.shape[-2])
    probs = torch.softmax(s.float(), dim=-1).to(qkv.dtype)
    if training and p > 0:
        probs = _phil_dropout(probs, p, training=True)
    o = probs @ v                        # (B, H, S, D)
    # token-major (B, S, H*D) like the fused kernel (the next Linear's
    # input layout)
    B, Hh, S, D = o.shape
    return o.transpose(1, 2).reshape(B, S, Hh * D)


class AttentionCoreQKV(nn.Module):
    """Fused flash-style attention over packed (B,S,3,H,D) qkv.

    prob_dropout: dropout rate applied to the ATTENTION PROBABILITIES
    (HF BertSelfAttention semantics). On the D=64 path the philox mask
    is FUSED into the flash fwd/bwd kernels (no P materialization;
    masks regenerated in the backward from the same counter scheme);
    other shapes route through the composed P-materializing path.
    Measured cost on BERT-base: ~19% step time (philox at 4 kernel
    sites), so prob_dropout == 0 remains the perf default used by the
    bench models, which apply dropout AFTER the output projection — a
    DOCUMENTED semantics difference vs HF BERT."""
    _is_leaf_module = True

    def __init__(self, causal: bool = False, prob_dropout: float = 0.0):
        super().__init__()
        self.causal = causal
        self.prob_dropout = prob_dropout

    def forward(self, qkv, mask=None, kv_len=None, cu_seqlens=None,
                tiles=None):
        if cu_seqlens is not None:
            # packed (T,3,H,D) token stream: the lengths are the mask
            if mask is not None or kv_len is not None \
                    or self.prob_dropout > 0:
                raise ValueError(
                    "cu_seqlens (varlen attention) cannot be combined with "
                    "mask, kv_len or prob_dropout > 0")
            return attention_varlen_qkv(qkv, cu_seqlens, causal=self.causal,
                                        tiles=tiles).flatten(1)
        if self.prob_dropout > 0 and self.training and qkv.is_cuda:
            if qkv.shape[-1] == 64:  # fused philox masks in the kernels
                return attention_qkv(qkv, mask=mask, causal=self.causal,
                                     prob_dropout=self.prob_dropout,
                                     kv_len=kv_len)
            return attention_qkv_prob_dropout(
                qkv, mask, self.causal, None, self.prob_dropout,
                self.training, kv_len)
        return attention_qkv(qkv, mask=mask, causal=self.causal,
                             kv_len=kv_len)


def varlen_tiles(cu_seqlens, T):
    """Tile table of the varlen attention kernels for one packed batch of T
    rows: int32 (T // 128 + B + 2, 2), built on the device from cu_seqlens
    (int32 (B+1,)) by one small kernel, no host read. Build it once per
    batch and hand it to every layer, forward and backward use the same
    one. None for CPU tensors (the composed twin needs no table)."""
    if not cu_seqlens.is_cuda:
        return None
    return get_ext(required=True).attn_varlen_tiles(cu_seqlens, T)


class _AttnVarlenFn(torch.autograd.Function):
    """Packed varlen path: qkv (T,3,H,64) -> o (T,H,64), per sequence of
    cu_seqlens (csrc/attention_varlen64.hip)."""

    @staticmethod
    def forward(ctx, qkv, cu_seqlens, tiles, causal, scale):
        ext = get_ext(required=True)
        o, lse = ext.attn_varlen_fwd_qkv(qkv, cu_seqlens, tiles, causal,
                                         scale)
        ctx.save_for_backward(qkv, o, lse, cu_seqlens, tiles)
        ctx.causal = causal
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, cu_seqlens, tiles = ctx.saved_tensors
        dqkv = get_ext(required=True).attn_varlen_bwd_qkv(
            qkv, o, do.contiguous(), lse, cu_seqlens, tiles, ctx.causal,
            ctx.scale)
        return dqkv, None, None, None, None


def _varlen_twin(qkv, cu_seqlens, causal, scale):
    """Composed form of the varlen kernels: every sequence through
    _math_attention, zeros on the tail. Reads cu_seqlens on the host."""
    T, _, H, D = qkv.shape
    cu = cu_seqlens.tolist()
    outs = []
    for lo, hi in zip(cu[:-1], cu[1:]):
        if hi > lo:
            q, k, v = (qkv[lo:hi, i].transpose(0, 1) for i in range(3))
            outs.append(_math_attention(q, k, v, None, causal,
                                        scale).transpose(0, 1))
    outs.append(qkv.new_zeros(T - cu[-1], H, D))
    return torch.cat(outs)


def attention_varlen_qkv(qkv, cu_seqlens, causal=False, scale=None,
                         tiles=None):
    """Attention within each sequence of a packed token stream.

    qkv (T,3,H,D), token-major (the qkv projection of (T,C) activations);
    cu_seqlens int32 (B+1,) on qkv's device: cu[0] = 0, non-decreasing,
    cu[B] <= T, sequence b = rows [cu[b], cu[b+1]). Returns o (T,H,D).
    Rows [cu[B], T) are a tail: their o and dqkv are exact zeros whatever
    they hold (NaN included), so T may be rounded up. causal puts the
    diagonal at each sequence's start. No mask, no kv_len, no probability
    dropout: the lengths are the mask.

    CUDA + bf16 + D == 64 runs csrc/attention_varlen64.hip, whose grids
    depend on shapes only (nothing reads a length on the host); tiles is
    varlen_tiles(cu_seqlens, T), built here when not given. Everything
    else runs the composed twin, which reads cu_seqlens on the host."""
    if qkv.dim() != 4 or qkv.shape[1] != 3:
        raise ValueError("qkv must be (T, 3, H, D)")
    if cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2 \
            or cu_seqlens.dtype != torch.int32 \
            or cu_seqlens.device != qkv.device:
        raise ValueError("cu_seqlens must be int32 of shape (B+1,) on the "
                         "device of qkv")
    D = qkv.shape[-1]
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if qkv.is_cuda and qkv.dtype == torch.bfloat16 and D == 64:
        if tiles is None:
            tiles = varlen_tiles(cu_seqlens, qkv.shape[0])
        return _AttnVarlenFn.apply(qkv.contiguous(), cu_seqlens.contiguous(),
                                   tiles, causal, scale)
    return _varlen_twin(qkv, cu_seqlens, causal, scale)


def unpad_batch(input_ids, attention_mask, targets=None, multiple=64):
    """(B,S) padded batch -> packed token stream for the varlen path.

    Meant for the HOST tensors a data loader produces, before the copy to
    the device (boolean indexing of device tensors would synchronise).
    Returns (ids (T,), position ids (T,), cu_seqlens int32 (B+1,), targets
    (T,) or None, T): the tokens with attention_mask != 0 in batch order,
    their column as position, and T = their count rounded up to
    `multiple` (at least `multiple`). The tail holds id 0, position 0 and
    target -100 (the ignore index)."""
    keep = attention_mask != 0
    B, S = input_ids.shape
    lens = keep.sum(1)
    live = int(lens.sum())
    T = max(-(-live // multiple), 1) * multiple
    cu = torch.zeros(B + 1, dtype=torch.int32, device=input_ids.device)
    cu[1:] = lens.cumsum(0)
    ids = input_ids.new_zeros(T)
    ids[:live] = input_ids[keep]
    pos = input_ids.new_zeros(T)
    pos[:live] = torch.arange(S, device=input_ids.device).expand(B, S)[keep]
    tgt = None
    if targets is not None:
        tgt = targets.new_full((T,), -100)
        tgt[:live] = targets[keep]
    return ids, pos, cu, tgt, T


def _decode_twin(qkv_new, k_cache, v_cache, cache_len, scale):
    """Composed torch form of csrc/attention_decode.hip, same semantics:
    row L = cache_len[b] of the caches takes the new token's k and v in
    place (nothing is stored for L outside [0, S_max)), the query attends
    rows [0, L], softmax in fp32. Rows past L never reach the result,
    whatever they hold."""
    S_max = k_cache.shape[2]
    q, k, v = qkv_new.unbind(1)                       # (B, H, D) each
    L = cache_len.long()
    ok = ((L >= 0) & (L < S_max))[:, None, None, None]
    Lc = L.clamp(0, S_max - 1)
    idx = Lc[:, None, None, None].expand(-1, k.shape[1], 1, k.shape[2])
    for cache, new in ((k_cache, k), (v_cache, v)):
        row = torch.where(ok, new[:, :, None, :], cache.gather(2, idx))
        cache.scatter_(2, idx, row)
    dead = torch.arange(S_max, device=L.device)[None, :] > Lc[:, None]
    dead = dead[:, None, :, None]                     # (B, 1, S_max, 1)
    kf = k_cache.float().masked_fill(dead, 0.0)
    vf = v_cache.float().masked_fill(dead, 0.0)
    s = (kf @ q.float()[..., None]) * scale           # (B, H, S_max, 1)
    p = torch.softmax(s.masked_fill(dead, float("-inf")), dim=2)
    o = (p * vf).sum(dim=2)                           # (B, H, D)
    return o.flatten(1).to(qkv_new.dtype)


def attention_decode(qkv_new, k_cache, v_cache, cache_len, scale=None,
                     max_len=None, n_split=None):
    """One cached decoding step for every head of a batch.

    qkv_new (B,3,H,D): the qkv projection of the one new token.
    k_cache, v_cache (B,H,S_max,D): contiguous, updated in place.
    cache_len (B,) int32 on the device of the caches: keys already cached
    per sequence; read on the device only, never changed here (the caller
    adds 1 once per step for all layers).
    Sequence b with L = cache_len[b]: the new k and v go to row L, the
    query attends rows [0, L]. L >= S_max stores nothing and leaves that
    output row unspecified. Returns o (B, H*D), the layout proj reads.

    max_len: host-side upper bound on L + 1 (None = S_max); n_split: split
    count, None = chosen from B*H and max_len. Both only steer how the
    kernel divides the keys. CUDA + bf16 + D in (64, 128) runs
    csrc/attention_decode.hip; everything else the composed twin.
    Inference only: raises if an input requires grad."""
    if any(t.requires_grad for t in (qkv_new, k_cache, v_cache)):
        raise RuntimeError("attention_decode is inference-only: run it "
                           "under torch.no_grad() on detached tensors")
    if qkv_new.dim() != 4 or qkv_new.shape[1] != 3:
        raise ValueError("qkv_new must be (B, 3, H, D)")
    B, _, H, D = qkv_new.shape
    if k_cache.shape != v_cache.shape or k_cache.dim() != 4 \
            or k_cache.shape[0] != B or k_cache.shape[1] != H \
            or k_cache.shape[3] != D:
        raise ValueError("k_cache and v_cache must be (B, H, S_max, D)")
    if cache_len.shape != (B,) or cache_len.dtype != torch.int32 \
            or cache_len.device != k_cache.device:
        raise ValueError(f"cache_len must be int32 of shape ({B},) on the "
                         "caches' device")
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if qkv_new.is_cuda and qkv_new.dtype == torch.bfloat16 \
            and k_cache.dtype == torch.bfloat16 and D in (64, 128):
        ext = get_ext(required=True)
        return ext.attn_decode(qkv_new.contiguous(), k_cache, v_cache,
                               cache_len, scale, max_len, n_split)
    with torch.no_grad():
        return _decode_twin(qkv_new, k_cache, v_cache, cache_len, scale)
