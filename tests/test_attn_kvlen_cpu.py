"""Per-sequence key lengths in attention: the CPU side.

kv_len_from_mask is the torch twin of the attn_mask_kv_len kernel and the
reference the GPU tests derive their lengths with; the composed attention
paths must give kv_len the meaning the kernels give it (-inf on columns
>= kv_len[b]); and deriving the bound from BERT's padding mask must not
move a single logit.
"""
import importlib

import pytest
import torch

attn_mod = importlib.import_module("ravnest_amd.ops.attention")

S = 16
DEAD = -10000.0

# (name, live key positions or None for "all", expected kv_len)
MASK_CASES = [
    ("all_live", None, S),
    ("right_padded", range(0, 5), 5),
    ("hole_in_prefix", [0, 1, 2, 6, 7], 8),
    ("live_after_dead_run", [9, 10], 11),
    ("all_dead", [], S),
    ("single_key", [0], 1),
]


def _mask_row(live):
    row = torch.full((S,), DEAD)
    if live is None:
        row[:] = 0.0
    else:
        row[list(live)] = 0.0
    return row


def test_kv_len_from_mask_cases():
    rows = torch.stack([_mask_row(live) for _, live, _ in MASK_CASES])
    want = torch.tensor([w for _, _, w in MASK_CASES], dtype=torch.int32)
    for m in (rows, rows.view(len(MASK_CASES), 1, 1, S)):
        got = attn_mod.kv_len_from_mask(m)
        assert got.dtype == torch.int32 and got.shape == (len(MASK_CASES),)
        assert torch.equal(got, want), (got, want)


def test_kv_len_from_mask_neg_inf_is_dead():
    m = torch.zeros(3, S)
    m[0, 7:] = float("-inf")
    m[1, :] = float("-inf")
    m[2, 3] = float("-inf")          # a hole: ignored
    got = attn_mod.kv_len_from_mask(m)
    assert got.tolist() == [7, S, S]


def _inf_mask(kv_len, n):
    cols = torch.arange(n)
    m = torch.zeros(len(kv_len), n)
    m[cols[None, :] >= kv_len[:, None]] = float("-inf")
    return m.view(len(kv_len), 1, 1, n)


@pytest.mark.parametrize("causal", [False, True])
def test_attention_cpu_kv_len_equals_inf_mask(causal):
    torch.manual_seed(0)
    B, H, n, D = 4, 2, 24, 8
    q, k, v = (torch.randn(B, H, n, D) for _ in range(3))
    kv_len = torch.tensor([1, 7, 23, 24])
    got = attn_mod.attention(q, k, v, causal=causal, kv_len=kv_len)
    want = attn_mod.attention(q, k, v, mask=_inf_mask(kv_len, n),
                              causal=causal)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
    # out-of-range lengths mean 1 and S
    got = attn_mod.attention(q, k, v, causal=causal,
                             kv_len=torch.tensor([0, 7, 23, n + 5]))
    assert torch.equal(got, want)
    # the module form takes it too
    core = attn_mod.AttentionCore(causal=causal)
    assert torch.equal(core(q, k, v, kv_len=kv_len), want)


@pytest.mark.parametrize("causal", [False, True])
def test_attention_qkv_cpu_kv_len_equals_inf_mask(causal):
    torch.manual_seed(1)
    B, n, H, D = 3, 20, 2, 8
    qkv = torch.randn(B, n, 3, H, D)
    kv_len = torch.tensor([20, 1, 13], dtype=torch.int32)
    got = attn_mod.attention_qkv(qkv, causal=causal, kv_len=kv_len)
    want = attn_mod.attention_qkv(qkv, mask=_inf_mask(kv_len.long(), n),
                                  causal=causal)
    assert got.shape == (B, n, H * D)
    assert torch.equal(got, want)
    core = attn_mod.AttentionCoreQKV(causal=causal)
    assert torch.equal(core(qkv, kv_len=kv_len), want)
    # the composed prob-dropout path (p = 0 here) means the same thing
    got = attn_mod.attention_qkv_prob_dropout(qkv, None, causal, None, 0.0,
                                              False, kv_len=kv_len)
    assert torch.equal(got, want)


def test_attention_cpu_kv_len_counts_keys_not_queries():
    torch.manual_seed(2)
    B, H, nq, nk, D = 2, 2, 5, 9, 8
    q = torch.randn(B, H, nq, D)
    k, v = torch.randn(B, H, nk, D), torch.randn(B, H, nk, D)
    kv_len = torch.tensor([7, 9])
    got = attn_mod.attention(q, k, v, kv_len=kv_len)
    want = attn_mod.attention(q, k, v, mask=_inf_mask(kv_len, nk))
    assert got.shape == (B, H, nq, D)
    assert torch.equal(got, want)


def test_kv_len_shape_is_checked():
    q = torch.randn(2, 1, 4, 8)
    with pytest.raises(ValueError):
        attn_mod.attention(q, q, q, kv_len=torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError):
        attn_mod.attention(q, q, q, kv_len=torch.tensor([1.0, 2.0]))


def test_provider_var_len_batches():
    from examples.bert.provider import SEQ, synthetic_batches
    fixed = synthetic_batches(100)
    var = synthetic_batches(100, var_len=True)
    assert all(bool(b["attention_mask"].all()) for b in fixed)
    lens = torch.cat([b["attention_mask"].sum(1) for b in var])
    assert lens.min() >= 16 and lens.max() <= SEQ and lens.unique().numel() > 8
    for b in var[:4]:
        am = b["attention_mask"]
        assert am.shape == b["input_ids"].shape == (am.shape[0], SEQ)
        # right-padded: the mask never goes back up
        assert (am[:, 1:] <= am[:, :-1]).all()
        assert (b["labels"][am == 0] == -100).all()
        assert (b["labels"][am == 1] != -100).any()
    # seeded
    again = synthetic_batches(100, var_len=True)
    assert torch.equal(again[3]["attention_mask"], var[3]["attention_mask"])


def test_bert_cpu_logits_unchanged_by_kv_skip(monkeypatch):
    from ravnest_amd.models import BertConfig, BertForMLM
    torch.manual_seed(0)
    model = BertForMLM(BertConfig.tiny(max_seq=32)).eval()
    B, n = 3, 32
    ids = torch.randint(0, model.cfg.vocab_size, (B, n))
    am = torch.zeros(B, n, dtype=torch.int64)
    for b, length in enumerate([32, 9, 1]):
        am[b, :length] = 1
    with torch.no_grad():
        monkeypatch.setattr(attn_mod, "KV_SKIP", True)
        on = model(ids, am)
        monkeypatch.setattr(attn_mod, "KV_SKIP", False)
        off = model(ids, am)
    assert torch.isfinite(on).all()
    assert torch.equal(on, off)
