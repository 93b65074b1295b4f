"""Flash attention backward at head dimension 128 (csrc/attention_bwd128.hip).

Reference: float64 torch attention on the same bf16 inputs,
softmax(Q K^T * scale + additive terms) V and its autograd gradients, with
-inf on columns >= kv_len[b]; q, k, v, dO ~ N(0,1) in bf16, fixed seed.

Metric, per batch row b and tensor (o, dq, dk, dv): max|x - ref| / max|ref|
over that sequence. Bound 1.5e-2 = 3 x the worst figure (0.0036-0.0050) of
a CPU model of the kernel's roundings (P and dS rounded to bf16, Delta
from the bf16 o, bf16 outputs, fp32 accumulation) against float64 on these
shapes; the margin covers __expf and accumulation order. A wrong fragment,
swizzle or stride gives errors of order 1. kv_len stays >= 2: at 1 the
reference dq is identically zero and the metric undefined.
"""
import functools
import importlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

attn_mod = importlib.import_module("ravnest_amd.ops.attention")

D = 128
SCALE = 1.0 / math.sqrt(D)
BOUND = 1.5e-2
EMPTY = torch.Tensor()

# (S, causal, mask lengths, kv_len, B, H)
CASES = {
    # one block, ragged last 32-tile, idle waves
    "s72-causal-kvlen": (72, True, None, (72, 40), 2, 2),
    # two 128-key blocks, the second with one live wave; both LDS slots wrap
    "s160-full": (160, False, None, None, 2, 2),
    # horizon on a 32-tile edge + 1, on the block edge + 1, full
    "s160-causal-kvlen": (160, True, None, (33, 129, 160), 3, 2),
    # additive (B,1,1,S) mask, -10000 past the lengths, no kv_len
    "s160-mask": (160, False, (33, 129, 160), None, 3, 2),
    # three blocks, zero-store early exit of whole dk/dv blocks
    "s288-causal-kvlen": (288, True, None, (2, 97, 288), 3, 2),
    # just past the S <= 2048 lse-in-LDS switch of the dv/dk kernels
    "s2080-lse-global": (2080, False, None, None, 1, 1),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ravnest_amd.ops import get_ext
    get_ext(required=True)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ext(dev):
    from ravnest_amd.ops import get_ext
    return get_ext(True)


def _randn(dev, *shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(device=dev,
                                               dtype=torch.bfloat16)


def _past(lens, S, dev, value):
    """(B,1,1,S) additive term: `value` on columns >= lens[b]."""
    dead = (torch.arange(S, device=dev)[None, :]
            >= torch.tensor(lens, device=dev)[:, None])
    add = torch.zeros(dead.shape, dtype=torch.float64, device=dev)
    return add.masked_fill_(dead, value)[:, None, None, :]


@functools.lru_cache(maxsize=None)
def _case(dev, name):
    """Inputs and the float64 reference of one case, computed once."""
    S, causal, mlens, kvl, B, H = CASES[name]
    q, k, v, do = _randn(dev, 4, B, H, S, D).unbind(0)
    mask = _past(mlens, S, dev, -10000.0).float() if mlens else None
    q64, k64, v64 = (t.double().requires_grad_() for t in (q, k, v))
    s = q64 @ k64.transpose(-2, -1) * SCALE
    if mask is not None:
        s = s + mask.double()
    if kvl is not None:
        s = s + _past(kvl, S, dev, float("-inf"))
    if causal:
        s = s + torch.triu(torch.full((S, S), float("-inf"), device=dev), 1)
    o64 = torch.softmax(s, dim=-1) @ v64
    ref = (o64.detach(),) + torch.autograd.grad(o64, (q64, k64, v64),
                                                do.double())
    kv_len = (torch.tensor(kvl, device=dev, dtype=torch.int32)
              if kvl else None)
    return q, k, v, do, mask, kv_len, causal, ref


def _assert_close(name, got, ref):
    worst = 0.0
    for label, x, r in zip(("o", "dq", "dk", "dv"), got, ref):
        err = ((x.double() - r).abs().flatten(1).amax(1)
               / r.abs().flatten(1).amax(1))
        print(f"{name} {label}: {[f'{e:.4f}' for e in err.tolist()]}")
        worst = max(worst, float(err.max()))
    assert worst < BOUND, f"{name}: worst relative error {worst:.4g}"


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("layout", ["separate", "packed"])
def test_entry_points_vs_float64(dev, ext, layout, name):
    """ext.attn_bwd / ext.attn_bwd_qkv at D = 128 with the forward's o and
    lse (both raise before this feature); the packed gradients are
    bit-identical to the separate-layout kernels' on the same values."""
    q, k, v, do, mask, kv_len, causal, ref = _case(dev, name)
    m = mask if mask is not None else EMPTY
    if layout == "separate":
        o, lse = ext.attn_fwd(q, k, v, m, causal, SCALE, kv_len)
        dq, dk, dv = ext.attn_bwd(q, k, v, o, do, lse, m, causal, SCALE,
                                  kv_len)
    else:
        qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).contiguous()
        o_p, lse = ext.attn_fwd_qkv(qkv, m, causal, SCALE, 0.0, 0, None,
                                    kv_len)[:2]
        dqkv = ext.attn_bwd_qkv(qkv, o_p, do.transpose(1, 2).contiguous(),
                                lse, m, causal, SCALE, 0.0, None, kv_len)
        o = o_p.transpose(1, 2)
        dq, dk, dv = (dqkv[:, :, i].transpose(1, 2) for i in range(3))
        sep = ext.attn_bwd(q, k, v, o.contiguous(), do, lse, m, causal,
                           SCALE, kv_len)
        for x, y in zip((dq, dk, dv), sep):
            assert torch.equal(x, y)
    _assert_close(f"{name}/{layout}", (o, dq, dk, dv), ref)
    if kv_len is not None:  # rows past the horizon: exact zeros
        for b, n in enumerate(kv_len.tolist()):
            assert not dk[b, :, n:].any() and not dv[b, :, n:].any()


def test_public_paths_reach_the_kernels(dev, ext, monkeypatch):
    """attention() and attention_qkv() at D = 128 return the kernels' own
    bits; with BWD_D128 off, attention() takes the composed backward."""
    q, k, v, do, _, kv_len, causal, _ = _case(dev, "s160-causal-kvlen")
    o, lse = ext.attn_fwd(q, k, v, EMPTY, causal, SCALE, kv_len)
    want = ext.attn_bwd(q, k, v, o, do, lse, EMPTY, causal, SCALE, kv_len)
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    attn_mod.attention(*leaves, causal=causal, kv_len=kv_len).backward(do)
    for t, w in zip(leaves, want):
        assert torch.equal(t.grad, w)
    qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).contiguous()
    do_p = do.transpose(1, 2).contiguous()
    o_p, lse_p = ext.attn_fwd_qkv(qkv, EMPTY, causal, SCALE, 0.0, 0, None,
                                  kv_len)[:2]
    want_p = ext.attn_bwd_qkv(qkv, o_p, do_p, lse_p, EMPTY, causal, SCALE,
                              0.0, None, kv_len)
    qkv.requires_grad_()
    attn_mod.attention_qkv(qkv, causal=causal, kv_len=kv_len).backward(
        do_p.flatten(2))
    assert torch.equal(qkv.grad, want_p)
    monkeypatch.setattr(attn_mod, "BWD_D128", False)
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    attn_mod.attention(*leaves, causal=causal, kv_len=kv_len).backward(do)
    assert not torch.equal(leaves[0].grad, want[0])


@pytest.mark.parametrize("flag", [True, False])
def test_backward_memory(dev, monkeypatch, flag):
    """B=1, H=2, S=2048: one fp32 (B,H,S,S) tensor is 32 MiB. The kernel
    path allocates ~3 MiB of gradients plus Delta; the composed path, run
    as the guard of the measurement itself, must exceed 32 MiB."""
    monkeypatch.setattr(attn_mod, "BWD_D128", flag)
    q, k, v = (t.requires_grad_()
               for t in _randn(dev, 3, 1, 2, 2048, D, seed=1).unbind(0))
    o = attn_mod.attention(q, k, v, causal=True)
    do = torch.randn_like(o)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    o.backward(do)
    torch.cuda.synchronize()
    rise = (torch.cuda.max_memory_allocated() - before) / 2**20
    print(f"BWD_D128={flag}: backward peak rise {rise:.1f} MiB")
    assert rise < 16 if flag else rise > 32


def test_ring_chunk_bwd_uses_kernel(dev, ext):
    """_chunk_bwd at D = 128 is ext.attn_bwd with the caller's global lse."""
    from ravnest_amd.parallel.ring_attention import _chunk_bwd
    q, k, v, do = _case(dev, "s160-full")[:4]
    o, lse = ext.attn_fwd(q, k, v, EMPTY, True, SCALE)
    lse_g = lse + 0.5       # as if other chunks held part of the weight
    got = _chunk_bwd(q, k, v, o, do, lse_g, None, True, SCALE)
    want = ext.attn_bwd(q, k, v, o, do, lse_g, EMPTY, True, SCALE)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
