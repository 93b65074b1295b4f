"""Flash attention forward at head dimension 64: the 64-key-stage kernel
(csrc/attention_fwd64.hip, FWD64 on) and the 32-key-tile kernel it
replaces (csrc/attention.hip, FWD64 off) on the same cases and bounds.

Reference: float64 softmax(Q K^T * scale + additive terms) V and its
logsumexp on the same bf16 inputs, with -inf on columns >= kv_len[b];
q, k, v ~ N(0,1) in bf16, fixed seed (the inputs of
tests/test_attn_bwd64_gpu.py, so the autograd case can use its bound).

Metrics: O, per batch row b: max|o - ref| / max|ref| over that sequence;
lse: max abs error over the finite entries.

Bounds = 3 x the worst figure of a CPU model of the kernels' roundings
(fp32 scores and sums, P rounded to bf16 before P V, bf16 O;
tools/attn_fwd_round_model.py) against float64 on exactly these cases:
O 3 x 0.00371 = 0.0111 (the cases range over 0.00189-0.00371), lse
3 x 3.08e-06 = 9.2e-06 (4.2e-07-4.7e-07, and 3.08e-06 where the scores
are 8 x larger). The margin covers the
hardware exp2/log2, the e^8 defer-max headroom and summation order. A
wrong fragment, swizzle, stride, mask group or stage index gives errors
of order 1. kv_len stays >= 1.
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
WORST_MODEL_O = 0.00371
WORST_MODEL_LSE = 3.08e-06
BOUND_O = 3 * WORST_MODEL_O
BOUND_LSE = 3 * WORST_MODEL_LSE
# gradients through the backward: the bound of tests/test_attn_bwd64_gpu.py
# (3 x 0.0057, tools/attn_bwd_round_model.py on these inputs)
BOUND_GRAD = 3 * 0.0057
EMPTY = torch.Tensor()

# (S, causal, mask lengths, kv_len, B, H, k rows scaled by 8)
CASES = {
    # one stage whose second sub-tile is dead, idle waves
    "s40": (40, False, None, None, 2, 2, None),
    # a full sub-tile + a ragged one in the second stage
    "s72": (72, False, None, None, 2, 2, None),
    # last stage half full, second slot used once
    "s96": (96, False, None, None, 2, 2, None),
    # two query blocks, the second with one live wave; both slots wrap
    "s160": (160, False, None, None, 2, 2, None),
    # the diagonal splits a stage
    "s160-causal": (160, True, None, None, 2, 2, None),
    # horizon just past the 32-tile, 64-stage and 128-block edges, and full
    "s160-kvlen": (160, False, None, (33, 65, 129, 160), 4, 2, None),
    # additive (B,1,1,S) mask, -10000 past the same lengths, no kv_len
    "s160-mask": (160, False, (33, 65, 129, 160), None, 4, 2, None),
    # causal and horizon together, three query blocks
    "s288-causal-kvlen": (288, True, None, (2, 97, 288), 3, 2, None),
    # scores 8 x larger on keys 96..127: the running max moves, and O is
    # rescaled, in the second stage's second sub-tile
    "s160-kscale": (160, False, None, None, 2, 2, (96, 128)),
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


def _past(lens, S, dev, value):
    """(B,1,1,S) additive term: `value` on columns >= lens[b]."""
    dead = (torch.arange(S, device=dev)[None, :]
            >= torch.tensor(lens, device=dev)[:, None])
    add = torch.zeros(dead.shape, dtype=torch.float64, device=dev)
    return add.masked_fill_(dead, value)[:, None, None, :]


def make_inputs(name, dev):
    """Seeded bf16 q, k, v, dO, the additive mask and kv_len of a case."""
    S, causal, mlens, kvl, B, H, kscale = CASES[name]
    g = torch.Generator(device="cpu").manual_seed(0)
    q, k, v, do = (torch.randn(4, B, H, S, D, generator=g)
                   .to(device=dev, dtype=torch.bfloat16).unbind(0))
    if kscale:
        k = k.clone()
        k[:, :, kscale[0]:kscale[1]] *= 8
    mask = _past(mlens, S, dev, -10000.0).float() if mlens else None
    kv_len = (torch.tensor(kvl, device=dev, dtype=torch.int32)
              if kvl else None)
    return q, k, v, do, mask, kv_len, causal


def additive_terms(name, mask, dev):
    """Everything added to the scaled scores, float64 (B or 1,1,S,S)."""
    S, causal, _, kvl = CASES[name][:4]
    add = torch.zeros(1, 1, S, S, dtype=torch.float64, device=dev)
    if mask is not None:
        add = add + mask.double()
    if kvl is not None:
        add = add + _past(kvl, S, dev, float("-inf"))
    if causal:
        add = add + torch.triu(
            torch.full((S, S), float("-inf"), device=dev), 1)
    return add


def reference(name, q, k, v, mask):
    """float64 o (B,H,S,D) and lse (B,H,S)."""
    s = (q.double() @ k.double().transpose(-2, -1) * SCALE
         + additive_terms(name, mask, q.device))
    return torch.softmax(s, dim=-1) @ v.double(), torch.logsumexp(s, dim=-1)


def o_errors(o, ref):
    """max|o - ref| / max|ref| per batch row."""
    return ((o.double() - ref).abs().flatten(1).amax(1)
            / ref.abs().flatten(1).amax(1))


def lse_error(lse, ref):
    """max abs error over the finite entries (the infinite ones agree)."""
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(lse), fin)
    return float((lse.double() - ref)[fin].abs().max())


@functools.lru_cache(maxsize=None)
def _case(dev, name):
    """Inputs and the float64 reference of one case, computed once."""
    q, k, v, do, mask, kv_len, causal = make_inputs(name, dev)
    return q, k, v, do, mask, kv_len, causal, reference(name, q, k, v, mask)


def _packed(q, k, v):
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).contiguous()


def _fwd(ext, layout, case, flag):
    """o (B,H,S,D) and lse (B,H,S) through one entry point and arm."""
    q, k, v, _, mask, kv_len, causal, _ = case
    m = mask if mask is not None else EMPTY
    if layout == "separate":
        return ext.attn_fwd(q, k, v, m, causal, SCALE, kv_len, flag)
    o, lse = ext.attn_fwd_qkv(_packed(q, k, v), m, causal, SCALE, 0.0, 0,
                              None, kv_len, flag)
    return o.transpose(1, 2), lse


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("fwd64", [True, False], ids=["fwd64", "keys32"])
def test_forward_vs_float64(dev, ext, fwd64, name):
    """Both arms against float64 under the one pair of bounds; the
    element-wise gap between the arms is printed; two calls of one arm
    give the same bits."""
    case = _case(dev, name)
    o, lse = _fwd(ext, "separate", case, fwd64)
    o2, lse2 = _fwd(ext, "separate", case, fwd64)
    oth_o, oth_lse = _fwd(ext, "separate", case, not fwd64)
    ref_o, ref_lse = case[7]
    eo = o_errors(o, ref_o)
    el = lse_error(lse, ref_lse)
    print(f"{name}/fwd64={fwd64} o: {[f'{e:.5f}' for e in eo.tolist()]} "
          f"lse: {el:.3g}; max |arm - other arm| o "
          f"{float((o.float() - oth_o.float()).abs().max()):.3g} lse "
          f"{float((lse - oth_lse).abs().max()):.3g}")
    assert float(eo.max()) < BOUND_O, f"{name}: O error {float(eo.max()):.4g}"
    assert el < BOUND_LSE, f"{name}: lse error {el:.4g}"
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("fwd64", [True, False], ids=["fwd64", "keys32"])
def test_packed_layout(dev, ext, fwd64, monkeypatch):
    """attention_qkv on (B,S,3,H,D): the bits of the arm that
    ops.attention.FWD64 names, inside the bounds."""
    case = _case(dev, "s288-causal-kvlen")
    q, k, v, _, _, kv_len, causal, (ref_o, ref_lse) = case
    monkeypatch.setattr(attn_mod, "FWD64", fwd64)
    got = attn_mod.attention_qkv(_packed(q, k, v), causal=causal,
                                 kv_len=kv_len)
    o, lse = _fwd(ext, "packed", case, fwd64)
    B, H, S, _ = q.shape
    assert torch.equal(got.view(B, S, H, D).transpose(1, 2), o)
    eo, el = o_errors(o, ref_o), lse_error(lse, ref_lse)
    print(f"packed/fwd64={fwd64} o: {[f'{e:.5f}' for e in eo.tolist()]} "
          f"lse: {el:.3g}")
    assert float(eo.max()) < BOUND_O and el < BOUND_LSE


def test_positional_call_takes_the_default(dev, ext):
    """ext.attn_fwd without the flag runs the 64-key stages."""
    case = _case(dev, "s160-mask")
    q, k, v, _, mask, _, causal, _ = case
    o, lse = ext.attn_fwd(q, k, v, mask, causal, SCALE)
    want_o, want_lse = _fwd(ext, "separate", case, True)
    assert torch.equal(o, want_o) and torch.equal(lse, want_lse)


def test_autograd_feeds_the_backward(dev, monkeypatch):
    """attention(...).backward with FWD64 on and off: the O and lse of
    either forward give gradients inside the backward's bound of the
    float64 gradients."""
    q, k, v, do, _, _, causal, _ = _case(dev, "s160-causal")
    q64, k64, v64 = (t.double().requires_grad_() for t in (q, k, v))
    s = (q64 @ k64.transpose(-2, -1) * SCALE
         + additive_terms("s160-causal", None, dev))
    ref = torch.autograd.grad(torch.softmax(s, dim=-1) @ v64,
                              (q64, k64, v64), do.double())
    grads = {}
    for flag in (True, False):
        monkeypatch.setattr(attn_mod, "FWD64", flag)
        leaves = [t.clone().requires_grad_() for t in (q, k, v)]
        attn_mod.attention(*leaves, causal=causal).backward(do)
        grads[flag] = [t.grad for t in leaves]
        for label, g, r in zip(("dq", "dk", "dv"), grads[flag], ref):
            err = o_errors(g, r)
            print(f"autograd/fwd64={flag} {label}: "
                  f"{[f'{e:.4f}' for e in err.tolist()]}")
            assert float(err.max()) < BOUND_GRAD
    for label, a, b in zip(("dq", "dk", "dv"), grads[True], grads[False]):
        print(f"autograd {label}: max |on - off| "
              f"{float((a.float() - b.float()).abs().max()):.3g}")
