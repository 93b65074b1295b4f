"""BertForMLM.forward_loss seam (CPU): where the sparse MLM head does not
apply, forward_loss declines and the engine helper computes exactly
criterion(model(...), targets); forward() keeps returning dense logits."""
import torch

from ravnest_amd import set_seed
from ravnest_amd.engine.fused_loss import model_loss
from ravnest_amd.models import BertConfig, BertForMLM
from ravnest_amd.ops import CrossEntropyLoss


def _setup():
    set_seed(3)
    cfg = BertConfig.tiny(max_seq=16, vocab_size=1002)
    cfg.dropout = 0.0
    model = BertForMLM(cfg)
    model.train()
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, cfg.vocab_size, (2, 16), generator=g)
    mask = torch.ones_like(ids)
    labels = ids.clone()
    labels[torch.rand(ids.shape, generator=g) > 0.3] = -100
    return cfg, model, ids, mask, labels


def test_forward_still_returns_dense_logits():
    cfg, model, ids, mask, _ = _setup()
    out = model(ids, mask)
    assert out.shape == (2, 16, cfg.vocab_size)


def test_forward_loss_declines_on_cpu_and_helper_matches_exactly():
    _, model, ids, mask, labels = _setup()
    crit = CrossEntropyLoss(-100)
    assert model.forward_loss(ids, mask, labels, crit) is None
    want = crit(model(ids, mask), labels)
    got = model_loss(model, crit, [ids, mask], labels)
    assert torch.equal(got, want)


def test_flag_off_helper_matches_exactly(monkeypatch):
    _, model, ids, mask, labels = _setup()
    crit = CrossEntropyLoss(-100)
    monkeypatch.setenv("RAVNEST_SPARSE_MLM_HEAD", "0")
    assert model.forward_loss(ids, mask, labels, crit) is None
    got = model_loss(model, crit, [ids, mask], labels)
    assert torch.equal(got, crit(model(ids, mask), labels))


def test_helper_without_forward_loss():
    lin = torch.nn.Linear(4, 3)
    x = torch.randn(5, 4)
    t = torch.randint(0, 3, (5,))
    crit = CrossEntropyLoss(-100)
    assert torch.equal(model_loss(lin, crit, [x], t), crit(lin(x), t))
