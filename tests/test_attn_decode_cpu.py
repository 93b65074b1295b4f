"""Cached decoding without a GPU: the composed twin of the decode
attention kernel against float64, and GPT.generate(use_cache=True) against
the uncached path at the reference's own sorter size."""
import pytest
import torch

import attn_decode_cases as dc
from ravnest_amd.models.gpt import GPT, GPTConfig
from ravnest_amd.ops import attention_decode


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("case", dc.CASES[:3], ids=dc.IDS[:3])
def test_twin_matches_float64(case, D):
    """fp32 twin on the poisoned caches; 1e-5 covers fp32 reassociation."""
    S_max, lens, n_split, max_len = case
    qkv, kc, vc, cache_len = dc.make_inputs(D, S_max, lens, torch.float32)
    ref = dc.reference(qkv, kc, vc, lens)
    kc0, vc0 = kc.clone(), vc.clone()
    o = attention_decode(qkv, kc, vc, cache_len, max_len=max_len,
                         n_split=n_split)
    assert o.shape == (dc.B, dc.H * D) and o.dtype == torch.float32
    errs = dc.row_errors(o, ref)
    print("row errors", errs)
    assert max(errs) <= 1e-5
    dc.assert_cache(kc, vc, kc0, vc0, qkv, lens)
    assert cache_len.tolist() == list(lens)


def _last_logits(model, **kw):
    """generate() with a hook that keeps each step's last-position logits."""
    steps = []
    hook = model.lm_head.register_forward_hook(
        lambda mod, inp, out: steps.append(out[:, -1].clone()))
    try:
        tokens = model.generate(**kw)
    finally:
        hook.remove()
    return tokens, torch.stack(steps)


def test_generate_cached_matches_uncached():
    torch.manual_seed(0)
    model = GPT(GPTConfig.nano(block_size=16)).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (2, 6))
    want, want_logits = _last_logits(model, idx=idx, max_new_tokens=6)
    got, got_logits = _last_logits(model, idx=idx, max_new_tokens=6,
                                   use_cache=True)
    assert got.shape == (2, 12) and torch.equal(got, want)
    assert got_logits.shape == want_logits.shape
    assert (got_logits - want_logits).abs().max().item() <= 1e-4
    with pytest.raises(ValueError):
        model.generate(idx, 11, use_cache=True)


def test_decode_rejects_grad():
    qkv, kc, vc, cache_len = dc.make_inputs(64, 64, (0, 1, 63),
                                            torch.float32)
    with pytest.raises(RuntimeError):
        attention_decode(qkv.requires_grad_(), kc, vc, cache_len)
