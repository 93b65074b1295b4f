"""DropoutAddLayerNorm without a GPU: the CPU fallback, checkpoint
compatibility of the BERT layers that use it, and fx tracing."""
import torch

from ravnest_amd import set_seed
from ravnest_amd.models import BertConfig, BertForMLM
from ravnest_amd.ops import (DropoutAddLayerNorm, add_layer_norm, dropout,
                             dropout_add_layer_norm)


def test_cpu_fallback_equals_composed_ops():
    torch.manual_seed(0)
    H = 48
    a = torch.randn(3, 7, H, requires_grad=True)
    z = torch.randn(3, 7, H, requires_grad=True)
    m = DropoutAddLayerNorm(H, 1e-5, 0.3)
    with torch.no_grad():
        m.weight.copy_(torch.randn(H))
        m.bias.copy_(torch.randn(H))
    dy = torch.randn(3, 7, H)

    st = torch.get_rng_state()
    y = m(a, z)
    y.backward(dy)
    got = (y.detach(), a.grad.clone(), z.grad.clone(), m.weight.grad.clone())
    after = torch.get_rng_state()

    a.grad = z.grad = None
    m.zero_grad()
    torch.set_rng_state(st)
    y2 = add_layer_norm(a, dropout(z, 0.3, True), m.weight, m.bias, 1e-5)
    y2.backward(dy)
    assert torch.equal(torch.get_rng_state(), after)
    for g, r in zip(got, (y2.detach(), a.grad, z.grad, m.weight.grad)):
        assert torch.equal(g, r)
    assert int((z.grad == 0).sum()) > 0  # dropout was active

    # eval mode and p = 0: plain add + LayerNorm, no RNG draw
    m.eval()
    st = torch.get_rng_state()
    y3 = m(a, z)
    assert torch.equal(torch.get_rng_state(), st)
    assert torch.equal(y3, add_layer_norm(a, z, m.weight, m.bias, 1e-5))
    assert torch.equal(
        dropout_add_layer_norm(a, z, m.weight, m.bias, 1e-5, 0.0, True), y3)


def _tiny(monkeypatch, flag):
    monkeypatch.setenv("RAVNEST_FUSED_DROPOUT_LN", flag)
    set_seed(0)
    return BertForMLM(BertConfig.tiny())


def test_bert_state_dict_same_with_flag_on_and_off(monkeypatch):
    on = _tiny(monkeypatch, "1")
    off = _tiny(monkeypatch, "0")
    assert on.layers[0].ln1.fused and not off.layers[0].ln1.fused
    sd_on, sd_off = on.state_dict(), off.state_dict()
    assert list(sd_on) == list(sd_off)
    for k in sd_on:
        assert sd_on[k].shape == sd_off[k].shape, k
    for i in range(on.cfg.layers):
        for ln in ("ln1", "ln2"):
            assert f"layers.{i}.{ln}.weight" in sd_on
            assert f"layers.{i}.{ln}.bias" in sd_on


def test_checkpoint_saved_with_flag_off_loads_with_it_on(monkeypatch,
                                                         tmp_path):
    off = _tiny(monkeypatch, "0")
    with torch.no_grad():
        for p in off.parameters():
            p.add_(0.25)
    torch.save(off.state_dict(), tmp_path / "bert.pt")
    on = _tiny(monkeypatch, "1")
    res = on.load_state_dict(torch.load(tmp_path / "bert.pt"), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for (k, p), q in zip(on.state_dict().items(), off.state_dict().values()):
        assert torch.equal(p, q), k
    # same weights, eval mode: both compute the same thing
    ids = torch.randint(0, on.cfg.vocab_size, (2, 16))
    mask = torch.ones_like(ids)
    on.eval(), off.eval()
    with torch.no_grad():
        assert torch.equal(on(ids, mask), off(ids, mask))


def test_fx_trace_keeps_module_as_leaf():
    from ravnest_amd.planner.splitter import (split_model_by_proportions,
                                              trace_model)
    set_seed(0)
    m = BertForMLM(BertConfig.tiny())
    gm = trace_model(m)
    leaves = [n for n in gm.graph.nodes if n.op == "call_module"
              and isinstance(gm.get_submodule(n.target), DropoutAddLayerNorm)]
    assert len(leaves) == 2 * m.cfg.layers
    assert all(len(n.args) == 2 for n in leaves)  # (residual, sublayer out)

    ids = torch.randint(0, m.cfg.vocab_size, (2, 16))
    mask = torch.ones_like(ids)
    m.eval()
    res = split_model_by_proportions(m, [0.5, 0.5], example_args=(ids, mask))
    assert len(res.stages) == 2
    with torch.no_grad():
        assert torch.allclose(res.split_gm(ids, mask), m(ids, mask),
                              atol=1e-6)
