"""Flash attention backward at head dimension 64: the 64-row-stage kernels
(csrc/attention_bwd64.hip, BWD64 on) and the 32-row kernels they replace
(csrc/attention_bwd.hip, BWD64 off) on the same cases and the same bound.

Reference: float64 torch attention on the same bf16 inputs,
softmax(Q K^T * scale + additive terms) V and its autograd gradients, with
-inf on columns >= kv_len[b]; q, k, v, dO ~ N(0,1) in bf16, fixed seed.

Metric, per batch row b and tensor (dq, dk, dv): max|x - ref| / max|ref|
over that sequence. Bound 0.0171 = 3 x the worst figure 0.0057 (the
cases range over 0.0023-0.0057) of a CPU model of the kernels' roundings (P and dS
rounded to bf16, Delta from the bf16 o, bf16 outputs, fp32 accumulation;
tools/attn_bwd_round_model.py) against float64 on exactly these cases;
the margin covers __expf and accumulation order. A wrong fragment, swizzle,
stride or stage index gives errors of order 1. kv_len stays >= 2: at 1 the
reference dq is identically zero and the metric undefined.
"""
import functools
import importlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

attn_mod = importlib.import_module("ravnest_amd.ops.attention")

D = 64
SCALE = 1.0 / math.sqrt(D)
WORST_MODEL = 0.0057
BOUND = 3 * WORST_MODEL
EMPTY = torch.Tensor()

# (S, causal, mask lengths, kv_len, B, H)
CASES = {
    # one stage whose second sub-tile is dead, idle waves
    "s40": (40, False, None, None, 2, 2),
    # a full sub-tile + a ragged one in the second stage
    "s72": (72, False, None, None, 2, 2),
    # odd number of 32-row tiles: last stage half full, second slot used once
    "s96": (96, False, None, None, 2, 2),
    # two 128-key blocks, the second with one live wave; both slots wrap
    "s160": (160, False, None, None, 2, 2),
    # diagonal tiles that split a stage
    "s160-causal": (160, True, None, None, 2, 2),
    # horizon just past the 32-tile, 64-stage and 128-block edges, and full
    "s160-kvlen": (160, False, None, (33, 65, 129, 160), 4, 2),
    # additive (B,1,1,S) mask, -10000 past the same lengths, no kv_len
    "s160-mask": (160, False, (33, 65, 129, 160), None, 4, 2),
    # three blocks, zero-store early exit of whole dk/dv blocks
    "s288-causal-kvlen": (288, True, None, (2, 97, 288), 3, 2),
    # just past the S <= 2048 lse/Delta-in-LDS switch
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


def make_inputs(name, dev):
    """Seeded bf16 q, k, v, dO, the additive mask and kv_len of a case."""
    S, causal, mlens, kvl, B, H = CASES[name]
    g = torch.Generator(device="cpu").manual_seed(0)
    q, k, v, do = (torch.randn(4, B, H, S, D, generator=g)
                   .to(device=dev, dtype=torch.bfloat16).unbind(0))
    mask = _past(mlens, S, dev, -10000.0).float() if mlens else None
    kv_len = (torch.tensor(kvl, device=dev, dtype=torch.int32)
              if kvl else None)
    return q, k, v, do, mask, kv_len, causal


def _past(lens, S, dev, value):
    """(B,1,1,S) additive term: `value` on columns >= lens[b]."""
    dead = (torch.arange(S, device=dev)[None, :]
            >= torch.tensor(lens, device=dev)[:, None])
    add = torch.zeros(dead.shape, dtype=torch.float64, device=dev)
    return add.masked_fill_(dead, value)[:, None, None, :]


def additive_terms(name, mask, dev):
    """Everything added to the scaled scores, float64 (B or 1,1,S,S)."""
    S, causal, _, kvl, _, _ = CASES[name]
    add = torch.zeros(1, 1, S, S, dtype=torch.float64, device=dev)
    if mask is not None:
        add = add + mask.double()
    if kvl is not None:
        add = add + _past(kvl, S, dev, float("-inf"))
    if causal:
        add = add + torch.triu(
            torch.full((S, S), float("-inf"), device=dev), 1)
    return add


def reference(name, q, k, v, do, mask):
    """float64 o, dq, dk, dv."""
    q64, k64, v64 = (t.double().requires_grad_() for t in (q, k, v))
    s = q64 @ k64.transpose(-2, -1) * SCALE + additive_terms(name, mask,
                                                             q.device)
    o64 = torch.softmax(s, dim=-1) @ v64
    return (o64.detach(),) + torch.autograd.grad(o64, (q64, k64, v64),
                                                 do.double())


def rel_errors(got, ref):
    """Per tensor: max|x - ref| / max|ref| per batch row."""
    return [((x.double() - r).abs().flatten(1).amax(1)
             / r.abs().flatten(1).amax(1)) for x, r in zip(got, ref)]


@functools.lru_cache(maxsize=None)
def _case(dev, name):
    """Inputs and the float64 reference of one case, computed once."""
    q, k, v, do, mask, kv_len, causal = make_inputs(name, dev)
    return q, k, v, do, mask, kv_len, causal, reference(name, q, k, v, do,
                                                        mask)


def _bwd(ext, layout, case, flag):
    """(dq, dk, dv) in (B,H,S,D) through one entry point and arm."""
    q, k, v, do, mask, kv_len, causal, _ = case
    m = mask if mask is not None else EMPTY
    if layout == "separate":
        o, lse = ext.attn_fwd(q, k, v, m, causal, SCALE, kv_len)
        return ext.attn_bwd(q, k, v, o, do, lse, m, causal, SCALE, kv_len,
                            flag)
    qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).contiguous()
    o_p, lse = ext.attn_fwd_qkv(qkv, m, causal, SCALE, 0.0, 0, None,
                                kv_len)[:2]
    dqkv = ext.attn_bwd_qkv(qkv, o_p, do.transpose(1, 2).contiguous(), lse,
                            m, causal, SCALE, 0.0, None, kv_len, flag)
    return [dqkv[:, :, i].transpose(1, 2) for i in range(3)]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("layout", ["separate", "packed"])
@pytest.mark.parametrize("bwd64", [True, False], ids=["bwd64", "rows32"])
def test_gradients_vs_float64(dev, ext, bwd64, layout, name):
    """Both arms against float64 under the one bound; rows past a kv_len
    horizon are exact zeros; the element-wise gap between the arms is
    printed per tensor."""
    case = _case(dev, name)
    got = _bwd(ext, layout, case, bwd64)
    other = _bwd(ext, layout, case, not bwd64)
    worst = 0.0
    for label, err, x, y in zip(("dq", "dk", "dv"),
                                rel_errors(got, case[7][1:]), got, other):
        gap = float((x.float() - y.float()).abs().max())
        print(f"{name}/{layout}/bwd64={bwd64} {label}: "
              f"{[f'{e:.4f}' for e in err.tolist()]} "
              f"max |arm - other arm| {gap:.3g}")
        worst = max(worst, float(err.max()))
    assert worst < BOUND, f"{name}: worst relative error {worst:.4g}"
    kv_len = case[5]
    if kv_len is not None:
        for b, n in enumerate(kv_len.tolist()):
            assert not got[1][b, :, n:].any() and not got[2][b, :, n:].any()


def test_switch_selects_the_kernels(dev, ext, monkeypatch):
    """attention() and attention_qkv() pass ops.attention.BWD64 on at call
    time: their gradients are the bits of the arm it names, and a
    positional ext.attn_bwd call (no flag) takes the default, stages on."""
    case = _case(dev, "s160-causal")
    q, k, v, do, _, _, causal, _ = case
    o, lse = ext.attn_fwd(q, k, v, EMPTY, causal, SCALE)
    default = ext.attn_bwd(q, k, v, o, do, lse, EMPTY, causal, SCALE)
    for flag in (True, False):
        monkeypatch.setattr(attn_mod, "BWD64", flag)
        want = _bwd(ext, "separate", case, flag)
        leaves = [t.clone().requires_grad_() for t in (q, k, v)]
        attn_mod.attention(*leaves, causal=causal).backward(do)
        for t, w in zip(leaves, want):
            assert torch.equal(t.grad, w)
        qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).contiguous()
        qkv.requires_grad_()
        attn_mod.attention_qkv(qkv, causal=causal).backward(
            do.transpose(1, 2).flatten(2))
        for i, w in enumerate(_bwd(ext, "packed", case, flag)):
            assert torch.equal(qkv.grad[:, :, i].transpose(1, 2), w)
        if flag:
            for x, w in zip(default, want):
                assert torch.equal(x, w)


def test_ring_chunk_bwd_takes_callers_lse(dev, ext):
    """_chunk_bwd at D = 64 is ext.attn_bwd with the caller's global lse,
    and both arms agree on it to within the bound."""
    from ravnest_amd.parallel.ring_attention import _chunk_bwd
    q, k, v, do = _case(dev, "s160")[:4]
    o, lse = ext.attn_fwd(q, k, v, EMPTY, True, SCALE)
    lse_g = lse + 0.5       # as if other chunks held part of the weight
    got = _chunk_bwd(q, k, v, o, do, lse_g, None, True, SCALE)
    want = ext.attn_bwd(q, k, v, o, do, lse_g, EMPTY, True, SCALE)
    old = ext.attn_bwd(q, k, v, o, do, lse_g, EMPTY, True, SCALE, None,
                       False)
    for x, y, z in zip(got, want, old):
        assert torch.equal(x, y)
        scale = float(z.float().abs().max())
        assert float((y.float() - z.float()).abs().max()) < BOUND * scale
