"""Delta = rowsum(dO * O) out of the D=64 dQ kernel (csrc/attention_bwd64.hip,
RAVNEST_ATTN_DELTA_FUSED=1; built, measured and left off by default, see
profiles/residual_delta.txt): the dq kernel computes its rows'
Delta from the dO fragments it holds and one read of O, stores it, and the
kv kernel, launched after it, reads it as before.

dq, dk, dv: against the float64 reference and under the bound of
tests/test_attn_bwd64_gpu.py (its reference, metric and BOUND are imported),
and against the RAVNEST_ATTN_DELTA_FUSED=0 arm (Delta kernel, kv, dq) in the
same process; the largest difference is printed.

Delta: the buffer handed to the backward against the float64 row sums of
the bf16 dO and the bf16 O the forward kernel wrote. The products of two
bf16 values are exact in fp32, so the error is that of adding D = 64 fp32
terms in some order: at most 64 * 2^-24 * sum_d |dO[d] * O[d]| per row. The
buffer is a slice of a larger one filled with a sentinel: nothing is stored
past row S - 1 of the last (batch, head).

Shapes (D = 64, B = 2, H = 2): S = 1 and 33 leave waves without rows, 64 is
one stage, 127 / 128 / 129 straddle the 128-row block, 200 has a ragged
second block, 512 is the flagship's length. Mask and kv_len variants end
the second sequence's keys at S // 2 + 1 (>= 2; there is none at S = 1).
At S = 1 the reference dq and dk are identically zero (one key: P = 1 and
dS = 0) and the imported metric, relative to max|ref|, is undefined; there
the error is taken relative to 1, the scale of the N(0,1) inputs.
"""
import functools
import math

import pytest
import torch

import test_attn_bwd64_gpu as base

pytestmark = pytest.mark.gpu

D, B, H = 64, 2, 2
SCALE = 1.0 / math.sqrt(D)
EMPTY = torch.Tensor()
SS = [1, 33, 64, 127, 128, 129, 200, 512]
VARIANTS = ["plain", "mask", "kvlen"]
CASES = [(S, layout, causal, variant) for S in SS
         for layout in ("separate", "packed") for causal in (False, True)
         for variant in VARIANTS if S > 1 or variant == "plain"]
PAD = 256
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ravnest_amd.ops import get_ext
    get_ext(required=True)
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(dev, S, causal, variant):
    """Inputs and the float64 reference of one case, computed once, through
    the case table of test_attn_bwd64_gpu."""
    lens = (S // 2 + 1, S)
    name = f"delta-{S}-{causal}-{variant}"
    base.CASES[name] = (S, causal, lens if variant == "mask" else None,
                        lens if variant == "kvlen" else None, B, H)
    q, k, v, do, mask, kv_len, _ = base.make_inputs(name, dev)
    return q, k, v, do, mask, kv_len, base.reference(name, q, k, v, do, mask)


def _run(ext, layout, case, causal):
    """(dq, dk, dv) in (B,H,S,D), Delta (B,H,S), the guard words behind it,
    and dO, O as (B,H,S,D) views."""
    q, k, v, do, mask, kv_len, _ = case
    S = q.shape[2]
    m = mask if mask is not None else EMPTY
    buf = torch.full((B * H * S + PAD,), SENTINEL, device=q.device)
    delta = buf[:B * H * S]
    if layout == "separate":
        o, lse = ext.attn_fwd(q, k, v, m, causal, SCALE, kv_len)
        grads = ext.attn_bwd(q, k, v, o, do, lse, m, causal, SCALE, kv_len,
                             True, delta)
    else:
        qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).contiguous()
        o_p, lse = ext.attn_fwd_qkv(qkv, m, causal, SCALE, 0.0, 0, None,
                                    kv_len)[:2]
        do_p = do.transpose(1, 2)       # (B,S,H,D) view of (B,H,S,D) memory
        assert not do_p.is_contiguous() or S == 1
        dqkv = ext.attn_bwd_qkv(qkv, o_p, do_p, lse, m, causal, SCALE, 0.0,
                                None, kv_len, True, delta)
        grads = [dqkv[:, :, i].transpose(1, 2) for i in range(3)]
        o = o_p.transpose(1, 2)
    torch.cuda.synchronize()
    return grads, delta.view(B, H, S).clone(), buf[B * H * S:].clone(), o


def _rel_errors(got, ref):
    """base.rel_errors, with 1 in place of a max|ref| of zero."""
    return [((x.double() - r).abs().flatten(1).amax(1)
             / r.abs().flatten(1).amax(1).masked_fill_(
                 r.abs().flatten(1).amax(1) == 0, 1.0))
            for x, r in zip(got, ref)]


@pytest.mark.parametrize("S,layout,causal,variant", CASES)
def test_fused_delta(dev, monkeypatch, S, layout, causal, variant):
    from ravnest_amd.ops import get_ext
    ext = get_ext(True)
    case = _case(dev, S, causal, variant)
    do = case[3]
    monkeypatch.setenv("RAVNEST_ATTN_DELTA_FUSED", "1")
    got, delta, guard, o = _run(ext, layout, case, causal)
    monkeypatch.setenv("RAVNEST_ATTN_DELTA_FUSED", "0")
    old, delta_old, guard_old, o_old = _run(ext, layout, case, causal)
    assert torch.equal(o, o_old)

    what = f"S={S}/{layout}/causal={causal}/{variant}"
    prod = do.double() * o.double()
    ref, bound = prod.sum(-1), 64 * 2.0 ** -24 * prod.abs().sum(-1)
    for arm, dl, gd in (("fused", delta, guard), ("kernel", delta_old,
                                                  guard_old)):
        err = (dl.double() - ref).abs()
        print(f"{what} Delta {arm}: max err {float(err.max()):.3e}  "
              f"max err/bound {float((err / bound.clamp(min=1e-30)).max()):.3f}"
              f"  max|Delta| {float(ref.abs().max()):.3e}")
        assert bool((err <= bound).all()), arm
        assert bool((gd == SENTINEL).all()), f"{arm}: stored past the rows"

    worst = 0.0
    for label, err, x, y in zip(("dq", "dk", "dv"),
                                _rel_errors(got, case[6][1:]), got, old):
        gap = float((x.float() - y.float()).abs().max())
        print(f"{what} {label}: {[f'{e:.4f}' for e in err.tolist()]} "
              f"max |fused - Delta-kernel arm| {gap:.3g}")
        worst = max(worst, float(err.max()))
    assert worst < base.BOUND, f"{what}: worst relative error {worst:.4g}"
    kv_len = case[5]
    if kv_len is not None:
        for b, n in enumerate(kv_len.tolist()):
            assert not got[1][b, :, n:].any() and not got[2][b, :, n:].any()
