"""Decode attention kernel (csrc/attention_decode.hip) against float64,
and cached generation against uncached generation, on the GPU."""
import pytest
import torch

import attn_decode_cases as dc
from ravnest_amd.models.gpt import GPT, GPTConfig
from ravnest_amd.ops import attention_decode

pytestmark = pytest.mark.gpu

# bf16 keeps 8 significand bits: unit roundoff 2**-8. fp32 part: sums of at
# most 2048 terms in numerator and denominator (2 * 2048 * 2**-24 = 2**-12)
# and __expf on arguments of a few units, together under 2**-11.
BOUND = 2.0 ** -8 + 2.0 ** -11


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_kernel_matches_float64(case, D):
    """Per batch row max|o - ref| / max|ref| <= BOUND on NaN-poisoned
    caches, and the cache rows afterwards.

    The bound was to be 2**-8 = twice a bf16 output rounding of 2**-9.
    The reference sanity check says otherwise: an fp32 torch model of the
    kernel's roundings (fp32 everywhere, one bf16 rounding of o) measures
    up to 3.69e-3 = 1.89 * 2**-9 on these cases, because the unit roundoff
    of bf16 is 2**-8, not 2**-9. Rederived: the output rounding gives at
    most 2**-8 in this metric (half an ulp of max|ref|'s binade over
    max|ref|), the fp32 arithmetic at most 2**-11 more (above). A wrong
    lane mapping, split merge or stride gives errors of order 1.
    Measured on an MI355X: worst row 3.69e-3 (D=128, S_max=64), the
    model's own figure; every row is also under 2**-8 = 3.91e-3."""
    S_max, lens, n_split, max_len = case
    qkv, kc, vc, cache_len = dc.make_inputs(D, S_max, lens, torch.bfloat16)
    ref = dc.reference(qkv, kc, vc, lens)
    dev = torch.device("cuda", 0)
    kc_d, vc_d = kc.to(dev), vc.to(dev)
    o = attention_decode(qkv.to(dev), kc_d, vc_d, cache_len.to(dev),
                         max_len=max_len, n_split=n_split)
    assert o.shape == (dc.B, dc.H * D) and o.dtype == torch.bfloat16
    errs = dc.row_errors(o, ref)
    print("row errors", errs)
    # a sequence past max_len is outside the contract: not compared
    live = [e for e, L in zip(errs, lens) if max_len is None or L < max_len]
    assert max(live) <= BOUND
    dc.assert_cache(kc_d, vc_d, kc, vc, qkv, lens)


def _last_logits(model, idx, steps, **kw):
    rows = []
    hook = model.lm_head.register_forward_hook(
        lambda mod, inp, out: rows.append(out[:, -1].double().cpu()))
    try:
        tokens = model.generate(idx, steps, **kw)
    finally:
        hook.remove()
    return tokens.cpu(), torch.stack(rows)


@pytest.mark.parametrize("name", ["nano64", "nano128"])
def test_generate_cached_no_worse_than_uncached(name):
    """Last-position logits of every step, cached and uncached, against a
    float64 CPU copy of the weights re-forwarding the tokens the uncached
    path chose: the cached path's worst max|logits - ref| / max|ref| is at
    most twice the uncached one's (the paths round differently: bf16 P in
    the flash kernel, fp32 p in the decode kernel). No token equality:
    near-ties may flip in bf16.
    Measured on an MI355X (uncached / cached): nano64 1.164e-2 / 1.111e-2,
    nano128 9.159e-3 / 1.167e-2 (profiles/attn_decode.txt)."""
    torch.manual_seed(0)
    cfg = getattr(GPTConfig, name)(vocab_size=64, block_size=32)
    dev = torch.device("cuda", 0)
    model = GPT(cfg).to(dev).to(torch.bfloat16).eval()
    ref_model = GPT(cfg).double().eval()
    ref_model.load_state_dict(model.state_dict())
    idx = torch.randint(0, cfg.vocab_size, (2, 5))
    tokens, plain = _last_logits(model, idx.to(dev), 8)
    _, cached = _last_logits(model, idx.to(dev), 8, use_cache=True)
    with torch.no_grad():
        ref = torch.stack([ref_model(tokens[:, :5 + i])[:, -1]
                           for i in range(8)])

    def worst(x):
        return ((x - ref).abs().amax((1, 2)) / ref.abs().amax((1, 2))).max()

    e_plain, e_cached = worst(plain).item(), worst(cached).item()
    print(f"{name}: uncached {e_plain:.3e} cached {e_cached:.3e}")
    assert e_cached <= 2 * e_plain
