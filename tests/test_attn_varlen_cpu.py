"""Varlen attention off the GPU: the composed twin against a per-sequence
float64 reference, unpad_batch, the packed BERT path against the padded
one, and the argument checks of AttentionCoreQKV."""
import pytest
import torch

import attn_varlen_cases as vc
from ravnest_amd import ops
from ravnest_amd.models import BertConfig, BertForMLM


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("tail", [0, 37])
@pytest.mark.parametrize("name", ["edges", "gaps"])
def test_twin_matches_float64(name, tail, causal):
    qkv, do, cu = vc.make_inputs(name, tail, dtype=torch.float32)
    qkv.requires_grad_()
    o = ops.attention_varlen_qkv(qkv, torch.tensor(cu, dtype=torch.int32),
                                 causal=causal)
    dqkv, = torch.autograd.grad(o, qkv, do)
    assert o.shape == do.shape
    assert (o[cu[-1]:] == 0).all() and (dqkv[cu[-1]:] == 0).all()
    nonempty = [(lo, hi) for lo, hi in zip(cu[:-1], cu[1:]) if hi > lo]
    for (lo, hi), ref in zip(nonempty, vc.reference(qkv.detach(), do, cu,
                                                    causal)):
        # fp32 round-off: sums of <= 288 products of O(1) terms
        assert vc.rel_err(o[lo:hi].transpose(0, 1), ref[0]) < 2e-5
        for i in range(3):
            assert vc.rel_err(dqkv[lo:hi, i].transpose(0, 1),
                              ref[2 + i]) < 2e-5


def _padded_batch(lens, S, vocab):
    torch.manual_seed(1)
    ids = torch.randint(1, vocab, (len(lens), S))
    mask = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()
    labelled = (torch.rand(len(lens), S) < 0.3) & (mask == 1)
    return ids * mask, mask, torch.where(labelled, ids, -100)


def test_unpad_batch():
    lens = (64, 17, 40)
    ids, mask, tgt = _padded_batch(lens, 64, 1024)
    pids, pos, cu, ptgt, T = ops.unpad_batch(ids, mask, tgt)
    assert T == 128 and pids.shape == pos.shape == ptgt.shape == (128,)
    assert cu.dtype == torch.int32 and cu.tolist() == [0, 64, 81, 121]
    for b, n in enumerate(lens):
        lo = cu[b]
        assert torch.equal(pids[lo:lo + n], ids[b, :n])
        assert torch.equal(ptgt[lo:lo + n], tgt[b, :n])
        assert torch.equal(pos[lo:lo + n], torch.arange(n))
    assert (pids[121:] == 0).all() and (pos[121:] == 0).all()
    assert (ptgt[121:] == -100).all()
    assert ops.unpad_batch(ids, mask, multiple=128)[4] == 128
    assert ops.unpad_batch(ids, mask, multiple=1)[4] == 121


def test_forward_packed_equals_forward():
    torch.manual_seed(2)
    model = BertForMLM(BertConfig.tiny()).eval()
    lens = (64, 17, 40)
    ids, mask, _ = _padded_batch(lens, 64, model.cfg.vocab_size)
    pids, pos, cu, _, _ = ops.unpad_batch(ids, mask)
    with torch.no_grad():
        dense = model(ids, mask)
        packed = model.forward_packed(pids, pos, cu)
    live = torch.cat([dense[b, :n] for b, n in enumerate(lens)])
    # logits are O(1); the two paths differ in fp32 summation order only
    assert (packed[:121] - live).abs().max() < 1e-5


@pytest.mark.parametrize("kw", [dict(mask=torch.zeros(1, 1, 1, 8)),
                                dict(kv_len=torch.tensor([8])),
                                dict(prob_dropout=0.1)])
def test_core_rejects_combinations(kw):
    core = ops.AttentionCoreQKV(prob_dropout=kw.pop("prob_dropout", 0.0))
    qkv = torch.randn(8, 3, 2, 64)
    cu = torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(ValueError):
        core(qkv, cu_seqlens=cu, **kw)
    assert ops.AttentionCoreQKV()(qkv, cu_seqlens=cu).shape == (8, 128)
